"""HIP-event time and achieved GB/s of bc_attention_ip (csrc/attention_ip.hip) at the four UNet levels of a 512^2 edit (canvas 64 x 128
latents), UNet batch 2 (one edit) and 16 (eight), with the base adapter's 4 image tokens.  Beside it the alternative with existing
launches - bc_attention at Nkv = 4 into a buffer of its own plus bc_add_rows onto the text attention's rows (two launches; the scale
would ride in V) - and, for scale, the launch it follows: attn2's text attention (bc_attention, 77 keys) on the same query rows.
Then the step time of the flagship 512^2 edit (bench.py's synthetic weights and inputs, batch 1) with one base adapter loaded (one
image, 1024-wide embeddings) beside the adapter-less step of the same build, alternating in one process: what the adapter costs with
attn2 on the forms that store q (no CHAIN_MIDX, no bc_ctx_fold) and 16 image-attention launches per UNet forward.

    python tools/ip_adapter_probe.py [--markdown profiles/ip_adapter.md] [--reps 20] [--steps 20] [--edits 4] [--no-step]

With --paths-markdown profiles/ip_adapter_plus.md [--only-paths] [--rounds 7]: the two kernels behind bc_attention_ip by name
(bc_attention_ip_with: the scalar kernel and the MFMA tiles) on the same eight shapes at T = 16, 32, 48 and 64 - the token counts of
IP-Adapter Plus with one to four images - alternating in one process, the dispatch rule read off that table, and the step time without an
adapter, with a base adapter and with a Plus adapter (ip-adapter-plus_sd15's shapes: 257 x 1280 hidden states, 16 queries).

With --masks-markdown profiles/ip_adapter_masks.md [--only-masks]: bc_attention_ip_masked (include/blobctrl_ip_mask.h) beside
bc_attention_ip at the four levels, UNet batch 2, for (images, tokens per image) = (1, 4), (2, 4), (1, 16), (4, 16), with a full mask and
with a blob-sized one (an ellipse over about a tenth of the canvas), every kernel by name and alternating in one process; the dispatch
rule of the masked kernels read off that table; the step time without an adapter, with a base adapter, and with the base adapter masked
by the blob; and what the bc_ip_mask_downsample launches of one edit cost.

Bytes are the algorithmic ones of the launch (Q read once, O read and written once, K and V once): 2 * (3 M C + 2 B T C).  Every launch
is replayed `reps` times in one segment behind a warm-up replay; the figure is the median of the per-launch event times.  Needs a GPU."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blobctrl_amd.launch import Recorder  # noqa: E402

LEVELS = ((320, 64 * 128), (640, 32 * 64), (1280, 16 * 32), (1280, 8 * 16))      # (channels, tokens per image)
HEADS, T_IP, T_TEXT = 8, 4, 77


def measure(dev, Cc, HW, B, reps):
    rec = Recorder(dev)
    try:
        d, M = Cc // HEADS, B * HW
        q, a = torch.randn(M, Cc, device=dev).half(), torch.randn(M, Cc, device=dev).half()
        k, v = torch.randn(B, T_IP, Cc, device=dev).half(), torch.randn(B, T_IP, Cc, device=dev).half()
        ck = torch.randn(B * T_TEXT, Cc, device=dev).half()
        cvt = torch.zeros(B, Cc, 128, device=dev).half()
        cvt[:, :, :T_TEXT] = torch.randn(B, Cc, T_TEXT, device=dev).half()
        w = torch.full((1,), 0.6, device=dev)
        vt4 = torch.zeros(B, Cc, 64, device=dev).half()                # the alternative's V^T [B][C][64], 4 keys, zero padded
        vt4[:, :, :T_IP] = v.transpose(1, 2)
        tmp, a2 = torch.empty_like(a), torch.empty_like(a)
        seg = rec.begin("probe")
        for _ in range(reps):
            rec.attention(q, ck, cvt, a, B, HEADS, d, HW, T_TEXT, Cc, Cc, 128, Cc, HW * Cc, T_TEXT * Cc, Cc * 128, HW * Cc, d ** -0.5)
            rec.attention_ip(q, k, v, a, B, HW, HEADS, d, T_IP, Cc, Cc, Cc, d ** -0.5, w)
            rec.attention(q, k, vt4, tmp, B, HEADS, d, HW, T_IP, Cc, Cc, 64, Cc, HW * Cc, T_IP * Cc, Cc * 64, HW * Cc, d ** -0.5)
            rec.call("bc_add_rows", a, tmp, M, M, Cc, a2, kind="add_rows", keep=(a, tmp, a2))
        s = torch.cuda.current_stream().cuda_stream
        seg.run(s)
        torch.cuda.synchronize()
        timed = seg.run_timed(s)
        ip = statistics.median(ms for m, ms in timed if m["kind"] == "attention_ip")
        att = [ms for m, ms in timed if m["kind"] == "attention"]
        text, alt = statistics.median(att[0::2]), statistics.median(att[1::2]) + statistics.median(ms for m, ms in timed if m["kind"] == "add_rows")
        nbytes = next(m["bytes"] for m, _ in timed if m["kind"] == "attention_ip")
        return ip * 1e3, nbytes / (ip * 1e-3) / 1e9, alt * 1e3, text * 1e3
    finally:
        rec.close()


PLUS_TOKENS = (16, 32, 48, 64)            # IP-Adapter Plus: 16 tokens per image; one to four images


def measure_paths(dev, Cc, HW, B, T, reps, rounds):
    """us per launch of both kernels behind bc_attention_ip (bc_attention_ip_with: path 0 scalar, path 1 MFMA tiles; T = 4 path 0 only) on
    one shape.  `reps` launches of a path are captured into one graph; the two graphs are replayed in turn, `rounds` times each behind a
    warm-up replay, in one process.  Returns {path: (median us, spread = max - min us over the rounds)} and the worst difference of the
    two paths' outputs on the same inputs."""
    from blobctrl_amd import _lib
    lib = _lib.load()
    d, M = Cc // HEADS, B * HW
    q, a0 = torch.randn(M, Cc, device=dev).half(), torch.randn(M, Cc, device=dev).half()
    k, v = torch.randn(B, T, Cc, device=dev).half(), torch.randn(B, T, Cc, device=dev).half()
    w = torch.full((1,), 0.6, device=dev)
    paths = (0, 1) if T % 16 == 0 else (0,)

    def launch(path, out):
        _lib.check(lib.bc_attention_ip_with(path, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, HW, HEADS, d, T, Cc, Cc, Cc,
                                            d ** -0.5, w.data_ptr(), torch.cuda.current_stream().cuda_stream), f"path {path}")
    outs = {}
    for p in paths:                                                    # one launch each on the same inputs: the results must agree
        outs[p] = a0.clone()
        launch(p, outs[p])
    torch.cuda.synchronize()
    diff = (outs[0].float() - outs[1].float()).abs().max().item() if len(paths) == 2 else 0.0
    return replay_in_turn({p: (lambda out, p=p: launch(p, out)) for p in paths}, a0, reps, rounds), diff


def paths_table(dev, reps, rounds):
    """The two-path table and the dispatch rule read off it: [markdown lines], {(C, T): tiles win on both batch rows beyond the spread}."""
    lines = ["# bc_attention_ip at 16 to 64 image tokens on an MI355X: the scalar kernel and the MFMA tiles", "",
             f"HIP-event time per launch: {reps} launches of one path captured into one graph, the two paths' graphs replayed in turn,",
             f"{rounds} replays each behind a warm-up, in one process.  us = median over the replays, +- = max - min over them (the run-to-run",
             "spread).  Both paths through bc_attention_ip_with on the same inputs; `max diff` is the largest difference of their fp16 outputs",
             "after one launch.  T = 4 is the base adapter on the scalar kernel: the anchor.", "",
             "| C | tokens / image | UNet batch | T | scalar us | +- | tiles us | +- | tiles / scalar | max diff | tiles win |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    wins = {}
    for B in (2, 16):
        for Cc, HW in LEVELS:
            for T in (T_IP,) + PLUS_TOKENS:
                res, diff = measure_paths(dev, Cc, HW, B, T, reps, rounds)
                (s_us, s_sp) = res[0]
                if 1 in res:
                    (t_us, t_sp) = res[1]
                    win = s_us - t_us > max(s_sp, t_sp)
                    wins.setdefault((Cc, T), []).append(win)
                    lines.append(f"| {Cc} | {HW} | {B} | {T} | {s_us:.1f} | {s_sp:.1f} | {t_us:.1f} | {t_sp:.1f} | {t_us / s_us:.2f} | {diff:.4f} | "
                                 f"{'yes' if win else 'no'} |")
                else:
                    lines.append(f"| {Cc} | {HW} | {B} | {T} | {s_us:.1f} | {s_sp:.1f} | - | - | - | - | - |")
                print(lines[-1], flush=True)
    rule = {key: all(v) for key, v in wins.items()}                    # (1280 channels: two levels x two batches = four rows)
    lines += ["", "## Dispatch rule", "",
              "A (channel width, T) class goes to the tiles only where they win on every row of that class above by more than the spread.  Every row has",
              f"{HEADS} heads, so a class is the (heads, d) pair that was measured: another head split of the same width stays on the scalar kernel.", "",
              "| C | " + " | ".join(f"T = {T}" for T in PLUS_TOKENS) + " |", "|---|" + "---|" * len(PLUS_TOKENS)]
    for Cc in sorted({c for c, _ in LEVELS}):
        lines.append(f"| {Cc} | " + " | ".join("tiles" if rule[(Cc, T)] else "scalar" for T in PLUS_TOKENS) + " |")
    return lines, rule


MASK_CASES = ((1, 4), (2, 4), (1, 16), (4, 16))      # (images, tokens per image)


def blob_mask(h, w, images, dev):
    """fp16 [images][h * w]: an ellipse over about a tenth of the h x w canvas, bicubic-downsampled from a 0 / 1 mask at 8 x the size (so
    its rim holds the small non-zero values a real mask has); every image gets the same blob."""
    from blobctrl_amd import ip_masks
    y, x = torch.meshgrid(torch.arange(8 * h, device=dev), torch.arange(8 * w, device=dev), indexing="ij")
    inside = (((y + 0.5) / (8 * h) - 0.5) / 0.25) ** 2 + (((x + 0.5) / (8 * w) - 0.7) / 0.127) ** 2 <= 1.0      # pi * .25 * .127 = 0.0997
    m = inside.to(torch.float32)[None].expand(images, -1, -1).contiguous()
    return ip_masks.downsample(m, h * w), float(inside.float().mean())


def replay_in_turn(launchers, a0, reps, rounds):
    """{name: launcher(out)} -> {name: (median us per launch, max - min us over the rounds)}: `reps` launches of a launcher captured into
    one graph, the graphs replayed in turn, `rounds` times each behind a warm-up replay, in one process."""
    graphs, bufs = {}, {}
    side = torch.cuda.Stream()
    for n, fn in launchers.items():
        bufs[n] = a0.clone()
        graphs[n] = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            fn(bufs[n])                                                # (warm: the code object is loaded before the capture)
            torch.cuda.synchronize()
            with torch.cuda.graph(graphs[n], stream=side):
                for _ in range(reps):
                    fn(bufs[n])
    times = {n: [] for n in launchers}
    for r in range(rounds + 1):
        for n in launchers:
            bufs[n].copy_(a0)                                          # (in place: keep the values where they started)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[n].replay()
            e1.record()
            torch.cuda.synchronize()
            if r:
                times[n].append(e0.elapsed_time(e1) * 1e3 / reps)
    return {n: (statistics.median(t), max(t) - min(t)) for n, t in times.items()}


def measure_masked(dev, Cc, h, wd, B, images, Tp, reps, rounds):
    """One shape: the unmasked launch (the dispatcher's kernel) and every masked kernel by name under a full and under a blob mask."""
    from blobctrl_amd import _lib
    lib = _lib.load()
    HW, T = h * wd, images * Tp
    d, M = Cc // HEADS, B * HW
    q, a0 = torch.randn(M, Cc, device=dev).half(), torch.randn(M, Cc, device=dev).half()
    k, v = torch.randn(B, T, Cc, device=dev).half(), torch.randn(B, T, Cc, device=dev).half()
    w = torch.full((1,), 0.6, device=dev)
    blob, share = blob_mask(h, wd, images, dev)
    masks = {"full": torch.ones(images, HW, device=dev).half(), "blob": blob}
    stream = lambda: torch.cuda.current_stream().cuda_stream

    def plain(out):
        _lib.check(lib.bc_attention_ip(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, HW, HEADS, d, T, Cc, Cc, Cc, d ** -0.5,
                                       w.data_ptr(), stream()), "bc_attention_ip")

    def masked(path, m):
        def fn(out):
            _lib.check(lib.bc_attention_ip_masked_with(path, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, HW, HEADS, d, images, Tp,
                                                       Cc, Cc, Cc, d ** -0.5, w.data_ptr(), m.data_ptr(), HW, stream()), f"masked path {path}")
        return fn
    launchers = {"unmasked": plain}
    for path in ((0, 1) if Tp % 16 == 0 else (0,)):
        for name, m in masks.items():
            launchers[(path, name)] = masked(path, m)
    rows = float((blob != 0).any(0).float().mean())
    return replay_in_turn(launchers, a0, reps, rounds), share, rows


def masks_table(dev, reps, rounds):
    B = 2
    lines = ["# bc_attention_ip_masked on an MI355X: ip_adapter_masks beside the unmasked launch", "",
             f"HIP-event time per launch: {reps} launches of one kernel captured into one graph, the graphs of a shape replayed in turn, {rounds}",
             "replays each behind a warm-up, in one process.  us = median over the replays, +- = max - min over them (the run-to-run spread).",
             f"UNet batch {B}, {HEADS} heads.  `unmasked` is bc_attention_ip at images x Tp keys (the kernel its dispatcher picks); the masked kernels",
             "go through bc_attention_ip_masked_with by name: path 0 the scalar kernel, path 1 the MFMA tiles (Tp a multiple of 16).  `full`: a mask",
             "of ones; `blob`: an ellipse over a tenth of the canvas, bicubic-downsampled to the level (rows with a non-zero mask: last column).", "",
             "| C | rows / image | images x Tp | unmasked us | +- | scalar full us | +- | scalar blob us | +- | tiles full us | +- | tiles blob us | +- | "
             "blob rows |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    wins, blob_cheaper = {}, []
    for Cc, HW in LEVELS:
        h = int(round((HW // 2) ** 0.5))
        for images, Tp in MASK_CASES:
            res, share, rows = measure_masked(dev, Cc, h, 2 * h, B, images, Tp, reps, rounds)
            cell = lambda key: f"{res[key][0]:.1f} | {res[key][1]:.1f}" if key in res else "- | -"
            lines.append(f"| {Cc} | {HW} | {images} x {Tp} | {cell('unmasked')} | {cell((0, 'full'))} | {cell((0, 'blob'))} | {cell((1, 'full'))} | "
                         f"{cell((1, 'blob'))} | {rows:.3f} |")
            print(lines[-1], flush=True)
            if (1, "full") in res:
                wins.setdefault((Cc, images * Tp), []).append(all(
                    res[(0, m)][0] - res[(1, m)][0] > max(res[(0, m)][1], res[(1, m)][1]) for m in ("full", "blob")))
            best = min(res[(p, "blob")][0] for p in (0, 1) if (p, "blob") in res)
            blob_cheaper.append((Cc, HW, images, Tp, best, res["unmasked"][0]))
    lines += ["", "## Dispatch rule of the masked kernels", "",
              "A (channel width, images x Tp) class with Tp a multiple of 16 goes to the tiles where they beat the masked scalar kernel on every",
              "measured row of the class, under the full and under the blob mask, by more than the spread.  Measured classes:", ""]
    for (Cc, T), v in sorted(wins.items()):
        lines.append(f"- C = {Cc}, {T} keys: {'tiles' if all(v) else 'scalar'} ({sum(v)} of {len(v)} rows won by the tiles)")
    lines += ["", "## A blob-sized mask against the unmasked launch", "",
              "| C | rows / image | images x Tp | best masked kernel, blob us | unmasked us | blob / unmasked |", "|---|---|---|---|---|---|"]
    for Cc, HW, images, Tp, best, un in blob_cheaper:
        lines.append(f"| {Cc} | {HW} | {images} x {Tp} | {best:.1f} | {un:.1f} | {best / un:.2f} |")
    return lines


def downsample_lines(dev, reps, rounds):
    """What the four bc_ip_mask_downsample launches of one edit and adapter cost: a 512 x 1024 mask (the canvas of a 512^2 edit) to the
    four levels, one image, from fp32 and from uint8."""
    from blobctrl_amd import ip_masks
    lines = ["", "## The downsampling launches of one edit (once per edit and adapter, outside the captured graph)", "",
             "| mask | dtype | four levels, us (median) | +- |", "|---|---|---|---|"]
    for dtype in (torch.float32, torch.uint8):
        m = (torch.rand(1, 512, 1024, device=dev) > 0.5).to(dtype)
        outs = [torch.empty(1, HW, device=dev).half() for _, HW in LEVELS]

        def run():
            for (_, HW), o in zip(LEVELS, outs):
                ip_masks.downsample(m, HW, out=o)
        run()
        torch.cuda.synchronize()
        ts = []
        for _ in range(rounds + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                run()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / reps)
        ts = ts[1:]
        lines.append(f"| 512 x 1024, 1 image | {str(dtype).replace('torch.', '')} | {statistics.median(ts):.1f} | {max(ts) - min(ts):.1f} |")
        print(lines[-1], flush=True)
    lines += ["", "(host-launched, not captured: the figure includes the four launches' host time.)"]
    return lines


def masked_step_setup(dev):
    """The flagship edit's engine with one base adapter at hand: (engine, adapter, inputs, score, {name: extra keywords of the call})."""
    import bench
    from blobctrl_amd import synth
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from blobctrl_amd.splat import splat_features
    from blobctrl_amd.weights import PackedTrunk, convert_ip_adapter, ip_adapter_on_device, ip_attn2_prefixes
    ucfg, bcfg = bench.full_configs()
    usd, bsd = bench.synth_weights()
    prefixes = ip_attn2_prefixes(usd.keys())
    shapes = {f"{1 + 2 * j}.to_{n}_ip.weight": (usd[bp + "attn2.to_k.weight"].shape[0], 768) for j, bp in enumerate(prefixes) for n in "kv"}
    sd = {"image_proj": synth.synth_state_dict({"proj.weight": (4 * 768, 1024), "proj.bias": (4 * 768,), "norm.weight": (768,), "norm.bias": (768,)}, 51),
          "ip_adapter": synth.synth_state_dict(shapes, 52)}
    adapter = ip_adapter_on_device(convert_ip_adapter(sd, prefixes, 768), dev)
    eng = BlobCtrlEngine(PackedTrunk(usd, dev, ucfg.block_out_channels), PackedTrunk(bsd, dev, bcfg.block_out_channels), ucfg, bcfg,
                         device=str(dev), scheduler="ddim")
    del usd, bsd
    h = w = 64
    inp = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in bench.synth_inputs(h, w).items()}
    score = splat_features(**inp["blob"], score_size=(h, w), return_d_score=True, device=str(dev))
    embeds = [torch.randn(2, 1, 1024, device=dev)]
    y, x = torch.meshgrid(torch.arange(512, device=dev), torch.arange(1024, device=dev), indexing="ij")
    blob = ((((y + 0.5) / 512 - 0.5) / 0.25) ** 2 + (((x + 0.5) / 1024 - 0.7) / 0.127) ** 2 <= 1.0).to(torch.uint8)[None, None]
    extras = {"none": {}, "base": dict(ip_adapter_image_embeds=embeds), "masked": dict(ip_adapter_image_embeds=embeds, ip_adapter_masks=[blob])}
    return eng, adapter, inp, score, extras


def masked_step_lines(dev, steps, edits):
    """ms per denoise step of the flagship edit without an adapter, with one base adapter, and with the base adapter masked by a blob."""
    import time
    eng, adapter, inp, score, extras = masked_step_setup(dev)

    def edit(name):
        eng.ip_adapters = [adapter] if name != "none" else []          # (the three plans have keys of their own and stay cached)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng(inp["prompt"], inp["fg"], inp["bg"], score, inp["dino"], num_inference_steps=steps, guidance_scale=7.5, latents=inp["latents"],
            **extras[name])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps
    names = ("none", "base", "masked")
    for n in names + names:                                            # record, capture, warm
        edit(n)
    times = {n: [] for n in names}
    for _ in range(edits):
        for n in names:
            times[n].append(edit(n))
    med = statistics.median
    row = lambda label, n: f"| {label} | {med(times[n]):.3f} | {' '.join(f'{v:.3f}' for v in times[n])} |"
    cost = lambda n, ref: f"{med(times[n]) - med(times[ref]):+.3f} ms per step ({100 * (med(times[n]) / med(times[ref]) - 1):+.1f} %)"
    return ["", f"## Step time, 512^2 edit, batch 1, DDIM, {steps} steps, whole-edit graph, alternating edits in one process", "",
            "| | ms per step (median) | every edit |", "|---|---|---|",
            row("no adapter", "none"), row("one base adapter, one image (T = 4), no mask", "base"),
            row("the same adapter, masked by a blob (a tenth of the 512 x 1024 canvas, uint8 on the device)", "masked"), "",
            f"Against no adapter the unmasked adapter costs {cost('base', 'none')}, the masked one {cost('masked', 'none')}; the mask changes the",
            f"adapter's step by {cost('masked', 'base')}.  The figure is the whole edit over its steps: the four downsampling launches of the",
            "masked edit, outside the graph, are inside it."]


def plus_adapter_shapes(embed=1280, hidden=768, ctx=768, queries=16, depth=4):
    """Parameter shapes of ip-adapter-plus_sd15's Resampler (ViT-H hidden states, 12 heads of 64) in the original key spelling."""
    shapes = {"latents": (1, queries, hidden), "proj_in.weight": (hidden, embed), "proj_in.bias": (hidden,), "proj_out.weight": (ctx, hidden),
              "proj_out.bias": (ctx,), "norm_out.weight": (ctx,), "norm_out.bias": (ctx,)}
    for i in range(depth):
        p = f"layers.{i}."
        shapes.update({p + "0.norm1.weight": (hidden,), p + "0.norm1.bias": (hidden,), p + "0.norm2.weight": (hidden,), p + "0.norm2.bias": (hidden,),
                       p + "0.to_q.weight": (hidden, hidden), p + "0.to_kv.weight": (2 * hidden, hidden), p + "0.to_out.weight": (hidden, hidden),
                       p + "1.0.weight": (hidden,), p + "1.0.bias": (hidden,), p + "1.1.weight": (4 * hidden, hidden),
                       p + "1.3.weight": (hidden, 4 * hidden)})
    return shapes


def step_times(dev, steps, edits):
    """ms per denoise step of the flagship edit without an adapter, with one base adapter and with one Plus adapter (one image each),
    alternating edits in one process: ({name: [ms]}, {name: launches per active step})."""
    import time
    import bench
    from blobctrl_amd import synth
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from blobctrl_amd.splat import splat_features
    from blobctrl_amd.weights import PackedTrunk, convert_ip_adapter, ip_adapter_on_device, ip_attn2_prefixes
    ucfg, bcfg = bench.full_configs()
    usd, bsd = bench.synth_weights()
    prefixes = ip_attn2_prefixes(usd.keys())
    shapes = {f"{1 + 2 * j}.to_{n}_ip.weight": (usd[bp + "attn2.to_k.weight"].shape[0], 768) for j, bp in enumerate(prefixes) for n in "kv"}
    sd = {"image_proj": synth.synth_state_dict({"proj.weight": (4 * 768, 1024), "proj.bias": (4 * 768,), "norm.weight": (768,), "norm.bias": (768,)}, 51),
          "ip_adapter": synth.synth_state_dict(shapes, 52)}
    sd_plus = {"image_proj": synth.synth_state_dict(plus_adapter_shapes(), 53), "ip_adapter": synth.synth_state_dict(shapes, 54)}
    adapters = {"base": ip_adapter_on_device(convert_ip_adapter(sd, prefixes, 768), dev),
                "plus": ip_adapter_on_device(convert_ip_adapter(sd_plus, prefixes, 768), dev)}
    eng = BlobCtrlEngine(PackedTrunk(usd, dev, ucfg.block_out_channels), PackedTrunk(bsd, dev, bcfg.block_out_channels), ucfg, bcfg,
                         device=str(dev), scheduler="ddim")
    del usd, bsd
    h = w = 64
    inp = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in bench.synth_inputs(h, w).items()}
    score = splat_features(**inp["blob"], score_size=(h, w), return_d_score=True, device=str(dev))
    embeds = {"base": [torch.randn(2, 1, 1024, device=dev)], "plus": [torch.randn(2, 1, 257, 1280, device=dev)]}
    ip_key = {"none": (), "base": (1,), "plus": ((1, 257),)}

    def edit(name):
        # (the three plans have keys of their own - no adapter, 4 tokens of 1024, 16 tokens of 257 x 1280 - and stay cached: nothing is dropped)
        eng.ip_adapters = [adapters[name]] if name != "none" else []
        extra = dict(ip_adapter_image_embeds=embeds[name]) if name != "none" else {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng(inp["prompt"], inp["fg"], inp["bg"], score, inp["dino"], num_inference_steps=steps, guidance_scale=7.5, latents=inp["latents"], **extra)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps
    names = ("none", "base", "plus")
    for n in names + names:                                            # record, capture, warm
        edit(n)
    times = {n: [] for n in names}
    for _ in range(edits):
        for n in names:
            times[n].append(edit(n))
    launches = {}
    for n in names:
        eng.ip_adapters = [adapters[n]] if n != "none" else []
        launches[n] = len(eng.plan_for(1, h, w, 77, 768, steps, ip=ip_key[n]).step_active)
    return times, launches


def step_lines(dev, steps, edits):
    times, launches = step_times(dev, steps, edits)
    med = statistics.median
    row = lambda label, n: f"| {label} | {med(times[n]):.3f} | {' '.join(f'{v:.3f}' for v in times[n])} | {launches[n]} |"
    cost = lambda n: f"{med(times[n]) - med(times['none']):+.3f} ms per step ({100 * (med(times[n]) / med(times['none']) - 1):+.1f} %)"
    return ["", f"## Step time, 512^2 edit, batch 1, DDIM, {steps} steps, whole-edit graph, alternating edits in one process", "",
            "| | ms per step (median) | every edit | launches per active step |", "|---|---|---|---|",
            row("no adapter", "none"), row("one base adapter, one image (T = 4)", "base"),
            row("one Plus adapter, one image (T = 16, 257 x 1280 hidden states)", "plus"), "",
            f"The base adapter costs {cost('base')}, the Plus adapter {cost('plus')}: 16 bc_attention_ip launches per UNet forward either",
            "way, and attn2 on the forms that store q (no CHAIN_MIDX at 320 / 640 channels, no bc_ctx_fold at 1280).  The figure is the",
            "whole edit over its steps, so the prologue - the Resampler, once per edit - is inside it.",
            "The adapter-less step records the launch list it recorded before adapters existed (tests/test_ip_adapter_cpu.py compares the",
            "listings): that is a statement about the listing, not a timing against the previous commit."]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markdown")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--edits", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--paths-markdown", help="time both kernels behind bc_attention_ip at T = 16, 32, 48, 64 and write the table there")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only-paths", action="store_true")
    ap.add_argument("--masks-markdown", help="time bc_attention_ip_masked beside bc_attention_ip, full and blob masks, and write the table there")
    ap.add_argument("--only-masks", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ip_adapter_probe needs an MI355X: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    if args.masks_markdown:                                            # profiles/ip_adapter_masks.md: the masked kernels, the rule, step and set-up cost
        mlines = masks_table(dev, args.reps, args.rounds) + downsample_lines(dev, args.reps, args.rounds)
        if not args.no_step:
            mlines += masked_step_lines(dev, args.steps, args.edits)
            for ln in mlines[-10:]:
                print(ln, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.masks_markdown)), exist_ok=True)
        with open(args.masks_markdown, "w") as f:
            f.write("\n".join(mlines) + "\n")
        if args.only_masks:
            return
    if args.paths_markdown:                                            # profiles/ip_adapter_plus.md: both kernels, the rule, the step cost
        plines, _ = paths_table(dev, args.reps, args.rounds)
        if not args.no_step:
            plines += step_lines(dev, args.steps, args.edits)
            for ln in plines[-12:]:
                print(ln, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.paths_markdown)), exist_ok=True)
        with open(args.paths_markdown, "w") as f:
            f.write("\n".join(plines) + "\n")
        if args.only_paths:
            return
    lines = ["# bc_attention_ip on an MI355X", "",
             f"HIP-event time per launch (median of {args.reps} replays in one segment), T = {T_IP} image tokens, {HEADS} heads; GB/s over the",
             "launch's algorithmic bytes 2 (3 M C + 2 B T C).  The alternative: bc_attention at Nkv = 4 into a buffer of its own + bc_add_rows",
             "(two launches).  For scale: attn2's text attention (bc_attention, 77 keys) on the same rows.", "",
             "| C | tokens / image | UNet batch | bc_attention_ip us | GB/s | bc_attention (Nkv = 4) + add us | text bc_attention us |",
             "|---|---|---|---|---|---|---|"]
    for B in (2, 16):
        for Cc, HW in LEVELS:
            us, gbs, alt_us, text_us = measure(dev, Cc, HW, B, args.reps)
            lines.append(f"| {Cc} | {HW} | {B} | {us:.1f} | {gbs:.0f} | {alt_us:.1f} | {text_us:.1f} |")
            print(lines[-1], flush=True)
    if not args.no_step:
        lines += step_lines(dev, args.steps, args.edits)
        for ln in lines[-12:]:
            print(ln, flush=True)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        with open(args.markdown, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
