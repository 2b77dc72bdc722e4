"""HIP-event time and achieved GB/s of bc_attention_ip (csrc/attention_ip.hip) at the four UNet levels of a 512^2 edit (canvas 64 x 128
latents), UNet batch 2 (one edit) and 16 (eight), with the base adapter's 4 image tokens.  Beside it the alternative with existing
launches - bc_attention at Nkv = 4 into a buffer of its own plus bc_add_rows onto the text attention's rows (two launches; the scale
would ride in V) - and, for scale, the launch it follows: attn2's text attention (bc_attention, 77 keys) on the same query rows.
Then the step time of the flagship 512^2 edit (bench.py's synthetic weights and inputs, batch 1) with one base adapter loaded (one
image, 1024-wide embeddings) beside the adapter-less step of the same build, alternating in one process: what the adapter costs with
attn2 on the forms that store q (no CHAIN_MIDX, no bc_ctx_fold) and 16 image-attention launches per UNet forward.

    python tools/ip_adapter_probe.py [--markdown profiles/ip_adapter.md] [--reps 20] [--steps 20] [--edits 4] [--no-step]

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


def step_times(dev, steps, edits):
    """ms per denoise step of the flagship edit without and with one adapter, alternating edits in one process: ([plain], [adapter])."""
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
    adapter = ip_adapter_on_device(convert_ip_adapter(sd, prefixes, 768), dev)
    eng = BlobCtrlEngine(PackedTrunk(usd, dev, ucfg.block_out_channels), PackedTrunk(bsd, dev, bcfg.block_out_channels), ucfg, bcfg,
                         device=str(dev), scheduler="ddim")
    del usd, bsd
    h = w = 64
    inp = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in bench.synth_inputs(h, w).items()}
    score = splat_features(**inp["blob"], score_size=(h, w), return_d_score=True, device=str(dev))
    embeds = [torch.randn(2, 1, 1024, device=dev)]

    def edit(with_adapter):
        eng.ip_adapters = [adapter] if with_adapter else []           # (both plans stay cached: nothing is dropped between edits)
        extra = dict(ip_adapter_image_embeds=embeds) if with_adapter else {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng(inp["prompt"], inp["fg"], inp["bg"], score, inp["dino"], num_inference_steps=steps, guidance_scale=7.5, latents=inp["latents"], **extra)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps
    for flag in (False, True, False, True):                            # record, capture, warm
        edit(flag)
    plain, ip = [], []
    for _ in range(edits):
        plain.append(edit(False))
        ip.append(edit(True))
    launches = {flag: len(eng.plan_for(1, h, w, 77, 768, steps, ip=(1,) if flag else ()).step_active) for flag in (False, True)}
    return plain, ip, launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markdown")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--edits", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ip_adapter_probe needs an MI355X: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
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
        plain, ip, launches = step_times(dev, args.steps, args.edits)
        med = statistics.median
        lines += ["", f"## Step time, 512^2 edit, batch 1, DDIM, {args.steps} steps, whole-edit graph, alternating edits in one process", "",
                  "| | ms per step (median) | every edit | launches per active step |", "|---|---|---|---|",
                  f"| no adapter | {med(plain):.3f} | {' '.join(f'{v:.3f}' for v in plain)} | {launches[False]} |",
                  f"| one adapter, one image | {med(ip):.3f} | {' '.join(f'{v:.3f}' for v in ip)} | {launches[True]} |", "",
                  f"The adapter costs {med(ip) - med(plain):+.3f} ms per step ({100 * (med(ip) / med(plain) - 1):+.1f} %): 16 bc_attention_ip launches per UNet",
                  "forward, and attn2 on the forms that store q (no CHAIN_MIDX at 320 / 640 channels, no bc_ctx_fold at 1280).",
                  "The adapter-less step records the launch list it recorded before adapters existed (tests/test_ip_adapter_cpu.py compares the",
                  "listings): that is a statement about the listing, not a timing against the previous commit."]
        for ln in lines[-11:]:
            print(ln, flush=True)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        with open(args.markdown, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
