#!/usr/bin/env python3
"""What stochastic DDIM costs per edit: 512^2, batch 1, 50 DDIM steps on bench.py's synthetic full-size setup, for eta = 0 and for
eta = 1 with a CPU generator and with generator=None (the device's global RNG).  Reports, per mode, the wall time of a whole edit
(`denoise`, host to result), the host time of drawing the per-step variance noise alone, and the replay time of the captured whole-edit
graph alone (device events around bc_graph_launch).

    python tools/eta_probe.py [EDITS]
"""
import ctypes as C
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def main():
    from blobctrl_amd import _lib
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from blobctrl_amd.splat import splat_features
    edits = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    dev = torch.device("cuda:0")
    h = w = 64
    n = 50
    ucfg, bcfg = bench.full_configs()
    usd, bsd = bench.synth_weights()
    inp = bench.synth_inputs(h, w, batch=1)
    score = splat_features(**inp["blob"], score_size=(h, w), return_d_score=True, device=str(dev))
    eng = BlobCtrlEngine(usd, bsd, ucfg, bcfg, device=str(dev), scheduler="ddim")
    lib = _lib.load()
    modes = [("eta=0", 0.0, None), ("eta=1, CPU generator", 1.0, "cpu"), ("eta=1, generator=None", 1.0, None)]
    print(f"512^2, batch 1, {n} DDIM steps, CFG 7.5; {edits} timed edits per mode after 2 warm-up edits")
    for name, eta, gdev in modes:
        def gen(i):
            return torch.Generator(device=gdev).manual_seed(1000 + i) if gdev else None

        def edit(i):
            return eng.denoise(inp["prompt"], inp["fg"], inp["bg"], score, inp["dino"], num_inference_steps=n, guidance_scale=7.5,
                               latents=inp["latents"], eta=eta, generator=gen(i) if eta else None)
        for i in range(2):
            edit(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(edits):
            edit(i)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / edits * 1e3
        # host time of the noise draws alone (what `denoise` adds in front of the replay), device work included
        draw = 0.0
        if eta:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(edits):
                BlobCtrlEngine.variance_noise(n, 1, h, w, gen(i), dev).to(dev)
            torch.cuda.synchronize()
            draw = (time.perf_counter() - t0) / edits * 1e3
        # the captured whole-edit graph alone
        P = eng.plan_for(1, h, w, inp["prompt"].shape[1], inp["prompt"].shape[2], n, stochastic=eta > 0)
        g = next(reversed(P.loop_graphs.values()))
        s = eng.stream.cuda_stream
        e0, e1 = C.c_void_p(), C.c_void_p()
        _lib.check(lib.bc_event_create(C.byref(e0)), "bc_event_create")
        _lib.check(lib.bc_event_create(C.byref(e1)), "bc_event_create")
        torch.cuda.synchronize()
        reps = []
        for _ in range(edits):
            with torch.cuda.stream(eng.stream):
                P.latents.copy_(inp["latents"].to(dev))
                P.hist.zero_()
                P.step_idx.zero_()
            _lib.check(lib.bc_event_record(e0, s), "bc_event_record")
            _lib.check(lib.bc_graph_launch(g, s), "bc_graph_launch")
            _lib.check(lib.bc_event_record(e1, s), "bc_event_record")
            eng.stream.synchronize()
            ms = C.c_float()
            _lib.check(lib.bc_event_elapsed_ms(e0, e1, C.byref(ms)), "bc_event_elapsed_ms")
            reps.append(ms.value)
        lib.bc_event_destroy(e0)
        lib.bc_event_destroy(e1)
        reps.sort()
        print(f"{name:24s} edit {wall:8.2f} ms | noise draw {draw:6.2f} ms ({n * 4 * h * w / 1e6:.2f} M floats) | "
              f"graph replay median {reps[len(reps) // 2]:8.2f} ms (min {reps[0]:.2f})", flush=True)
    print("cache:", eng.cache_stats)


if __name__ == "__main__":
    main()
