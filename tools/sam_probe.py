#!/usr/bin/env python3
"""HIP-event times of the Segment-Anything path at real ViT-H shape (synthetic weights: the arithmetic and the launches are those of the
released checkpoint):
  * `set_image`'s encoder replay and the implied fraction of the 2500 TFLOP/s fp16 peak against the derived 5.5 TFLOP of the encoder;
  * one `predict` (decoder replay + the two resizes);
  * bc_attention_relpos alone at the windowed shape (25 windows x 196 keys) and the global shape (4096 keys), 16 heads of 80, beside
    bc_attention on the same operands.
Prints one JSON line.  --layers N runs a shallower encoder (default 32)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ENCODER_TFLOP = 5.5          # derived by count (32 layers of projections + MLP over 4096 / 4900 tokens, four 4096-key attentions)
PEAK_TFLOPS = 2500.0


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), float(min(out))


def attention_pair(lib, check, B, side, heads=16, d=80, reps=20):
    """(relpos ms, plain ms) on the same Q | K buffer and V^T, model layout."""
    N, D = side * side, heads * d
    ldvt = (N + 63) // 64 * 64
    gen = torch.Generator(device="cuda").manual_seed(1)
    qk = torch.randn(B, N, 2 * D, generator=gen, device="cuda", dtype=torch.float16)
    vt = torch.zeros(B, D, ldvt, device="cuda", dtype=torch.float16)
    vt[:, :, :N] = torch.randn(B, D, N, generator=gen, device="cuda", dtype=torch.float16)
    rh = (torch.randn(2 * side - 1, d, generator=gen, device="cuda") / d ** 0.5).half()
    rw = (torch.randn(2 * side - 1, d, generator=gen, device="cuda") / d ** 0.5).half()
    o = torch.empty(B, N, D, device="cuda", dtype=torch.float16)
    rel = torch.empty(B * heads * N * 2 * side, device="cuda", dtype=torch.float32)
    s = torch.cuda.current_stream().cuda_stream
    args = (B, heads, d)
    strides = (2 * D, 2 * D, ldvt, D, N * 2 * D, N * 2 * D, D * ldvt, N * D, d ** -0.5)

    def relpos():
        check(lib.bc_attention_relpos(qk.data_ptr(), qk.data_ptr() + 2 * D, vt.data_ptr(), o.data_ptr(), *args, side, side, side, side,
                                      *strides, rh.data_ptr(), rw.data_ptr(), rel.data_ptr(), s), "bc_attention_relpos")

    def plain():
        check(lib.bc_attention(qk.data_ptr(), qk.data_ptr() + 2 * D, vt.data_ptr(), o.data_ptr(), *args, N, N, *strides, s), "bc_attention")

    return timed(relpos, reps), timed(plain, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from blobctrl_amd import _lib, synth
    from blobctrl_amd.sam import SamConfig, SamModel, SamPredictor
    lib = _lib.load()
    res = {"layers": args.layers}
    for name, B, side in (("windowed_25x196", 25, 14), ("global_4096", 1, 64)):
        (r_med, r_min), (p_med, p_min) = attention_pair(lib, _lib.check, B, side)
        flop = 4.0 * B * 16 * (side * side) ** 2 * 80
        res[name] = dict(relpos_ms=round(r_med, 4), relpos_min_ms=round(r_min, 4), plain_ms=round(p_med, 4), plain_min_ms=round(p_min, 4),
                         ratio=round(r_med / p_med, 3), relpos_tflops=round(flop / r_med * 1e-9, 1))
    glob = (7, 15, 23, 31) if args.layers == 32 else tuple(range(3, args.layers, 4))
    sd = synth.synth_state_dict(synth.sam_param_shapes(layers=args.layers, global_attn_indexes=glob), 131)
    model = SamModel(sd, SamConfig(num_heads=16, window_size=14, global_attn_indexes=glob))
    pred = SamPredictor(model)
    rng = np.random.Generator(np.random.PCG64(5))
    image = rng.integers(0, 256, size=(768, 1024, 3), dtype=np.uint8)
    pred.set_image(image)                                             # (planning + capture)
    P = model._encoder_plan(1)
    from blobctrl_amd.launch import run_graphed
    enc_med, enc_min = timed(lambda: run_graphed(P.seg, model.device), args.reps)
    pts, labs = np.array([[500.0, 375.0]]), np.array([1])
    pred.predict(pts, labs, multimask_output=False)                   # (planning + capture)
    frame_pts = np.array([[500.0, 375.0]], dtype=np.float32)

    def one_predict():
        low, _ = model.decode(frame_pts, labs, False)
        model.postprocess(low, pred.input_size, pred.original_size)

    pr_med, pr_min = timed(one_predict, args.reps)
    tflop = ENCODER_TFLOP * args.layers / 32
    res.update(encoder_ms=round(enc_med, 3), encoder_min_ms=round(enc_min, 3), encoder_launches=len(P.seg),
               encoder_tflops=round(tflop / enc_med * 1e3, 1), encoder_fraction_of_peak=round(tflop / enc_med * 1e3 / PEAK_TFLOPS, 4),
               recorded_gemm_attention_tflop=round(P.seg.flops * 1e-12, 3),
               predict_ms=round(pr_med, 3), predict_min_ms=round(pr_min, 3), predict_over_set_image=round(pr_med / enc_med, 4))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
