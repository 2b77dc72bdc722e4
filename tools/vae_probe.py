"""Time the full-size SD-1.5 VAE (encode 512^2 / decode 64x64 latent) on the HIP path and print the per-kernel event table.
PROBE_TILED=1: plain against tiled decode of a 96 x 96 latent (768^2: 2 x 2 tiles at the default 512 / 64 tile sizes) with HIP events,
and the blend kernel alone per tile: bytes from the shapes over the time of back-to-back launches."""
import sys
import os
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blobctrl_amd import synth                       # noqa: E402
from blobctrl_amd.vae import AutoencoderKL           # noqa: E402


def _events(fn, n):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def blend_bytes(t, B, C=3, src_bytes=4, out_bytes=4):
    """Bytes one blend launch has to move: the tile in, the keep-buffer out, the cropped part into the result, the neighbours' bands in."""
    n = t["out_h"] * t["out_w"] * (src_bytes + 4) + t["ch"] * t["cw"] * out_bytes + (t["ev"] * t["out_w"] + t["eh"] * t["out_h"]) * 4
    return B * C * n


def probe_tiled():
    from blobctrl_amd import _lib
    hw = int(sys.argv[1]) // 8 if len(sys.argv) > 1 else 96
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    vae = AutoencoderKL(synth.synth_state_dict(synth.vae_param_shapes(), 33))
    z = torch.randn(B, 4, hw, hw).cuda()
    times = {}
    for rep in range(2):                                  # plain and tiled alternate: both see the same machine
        for name, on in (("plain", False), ("tiled", True)):
            vae.enable_tiling(on)
            for _ in range(3):
                vae.decode(z)
            times.setdefault(name, []).append(_events(lambda: vae.decode(z), 10))
    for name, ts in times.items():
        print(f"decode latent {hw}x{hw} batch {B} {name}: " + ", ".join(f"{t:.3f}" for t in ts) + " ms per call (10 calls each)")
    geo = vae._tiles("decode", hw, hw)
    print(f"tiles: {geo['rows']} x {geo['cols']}, blend extent {geo['extent']}, crop {geo['limit']}, result {geo['out_h']}x{geo['out_w']}")
    out = torch.empty(B, 3, geo["out_h"], geo["out_w"], device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    keeps = {}
    for t in geo["tiles"]:
        src = torch.randn(B, t["out_h"], t["out_w"], 3, device="cuda")
        keep = torch.empty_like(src)
        above, left = keeps.get((t["i"] - 1, t["j"])), keeps.get((t["i"], t["j"] - 1))

        def launch():
            _lib.check(vae.lib.bc_vae_tile_blend(src.data_ptr(), above.data_ptr() if above is not None else None,
                                                 left.data_ptr() if left is not None else None, keep.data_ptr(), out.data_ptr(), 0, B,
                                                 t["out_h"], t["out_w"], above.shape[1] if above is not None else 0,
                                                 left.shape[2] if left is not None else 0, t["ev"], t["eh"], t["oy"], t["ox"], t["ch"],
                                                 t["cw"], geo["out_h"], geo["out_w"], s), "bc_vae_tile_blend")
        for _ in range(5):
            launch()
        ms = _events(launch, 200)
        keeps[(t["i"], t["j"])] = keep
        nbytes = blend_bytes(t, B)
        print(f"  blend tile ({t['i']}, {t['j']}) {t['out_h']}x{t['out_w']} ev {t['ev']} eh {t['eh']}: {ms * 1e3:.2f} us per launch "
              f"(200 back-to-back), {nbytes / 1e6:.2f} MB -> {nbytes / (ms * 1e-3) / 1e9:.0f} GB/s")


def main():
    if os.environ.get("PROBE_TILED"):
        return probe_tiled()
    res = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 1          # images per call (scripts/blobctrl_inference.py decodes num_samples = 2 at once)
    sd = synth.synth_state_dict(synth.vae_param_shapes(), 33)
    vae = AutoencoderKL(sd)
    z = torch.randn(B, 4, res // 8, res // 8).cuda()
    x = torch.randn(1, 3, res, res).clamp(-1, 1).cuda()
    for name, fn in (("decode", lambda: vae.decode(z)), ("encode", lambda: vae.encode(x))):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(10):
            fn()
        b.record()
        torch.cuda.synchronize()
        print(f"{name} {res}x{res} batch {z.shape[0] if name == 'decode' else 1}: {a.elapsed_time(b) / 10:.3f} ms")
    for key, P in vae._plans.items():
        rows = P.seg.run_timed(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        rows = P.seg.run_timed(torch.cuda.current_stream().cuda_stream)
        agg = {}
        for m, ms in rows:
            k = (m["kind"], m["variant"], str(m["shape"]))
            e = agg.setdefault(k, [0, 0.0, 0])
            e[0] += 1
            e[1] += ms
            e[2] += m["flops"]
        tot = sum(ms for _, ms in rows)
        print(f"--- {key}: {len(rows)} launches, {tot:.3f} ms serial, {P.seg.flops / 1e12:.3f} TFLOP")
        for k, e in sorted(agg.items(), key=lambda kv: -kv[1][1])[:18]:
            tf = e[2] / (e[1] * 1e-3) / 1e12 if e[1] > 0 else 0
            print(f"  {e[1]:8.3f} ms  x{e[0]:<3d} {tf:7.1f} TF/s  {k[0]:12s} {k[1]:50s} {k[2]}")


if __name__ == "__main__":
    main()
