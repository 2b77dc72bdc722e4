#!/usr/bin/env python3
"""One process of the FreeU A/B at 512^2, batch 1, the default scheduler (UniPC), 50 steps (the FreeU row): run it from the
root of a tree - the working tree, or a tree of the previous commit kept under _prev - and alternate the two on one box.

    python tools/freeu_ab.py TAG OUT_JSON        TAG = prev (a tree without FreeU) | cur

prev: the edit as every call before FreeU ran it.  cur: the same edit with FreeU off and with FreeU on (0.9, 0.2, 1.5, 1.6),
alternating.  Writes ms per edit and per step of every round, the launch counts of every plan, the final latents beside OUT_JSON (prev
and cur / off must be bit-identical) and, for the FreeU plan, the six launches' own times from the per-launch HIP-event table of one
active step (launches run back to back)."""
import json, os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
import torch
import bench
from blobctrl_amd.pipeline import BlobCtrlEngine
from blobctrl_amd.weights import PackedTrunk
from blobctrl_amd.splat import splat_features

tag, out_path = sys.argv[1], sys.argv[2]
STEPS, EDITS, ROUNDS = 50, 3, 4
FREEU = (0.9, 0.2, 1.5, 1.6)
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
ucfg, bcfg = bench.full_configs()
usd, bsd = bench.synth_weights()
pw_u, pw_b = PackedTrunk(usd, dev, ucfg.block_out_channels), PackedTrunk(bsd, dev, bcfg.block_out_channels)
del usd, bsd
h = w = 64
inp = bench.synth_inputs(h, w, batch=1)
inp = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}
score = splat_features(**inp["blob"], score_size=(h, w), return_d_score=True, device=str(dev))
eng = BlobCtrlEngine(pw_u, pw_b, ucfg, bcfg, device=str(dev), scheduler="unipc")


def edit(**kw):
    return eng.denoise(inp["prompt"], inp["fg"], inp["bg"], score, inp["dino"], num_inference_steps=STEPS, guidance_scale=7.5,
                       latents=inp["latents"], **kw)


modes = {"off": lambda: edit()} if tag == "prev" else {"off": lambda: edit(), "on": lambda: edit(freeu=FREEU)}
res = {"tag": tag, "steps": STEPS, "ms_per_edit": {m: [] for m in modes}}
finals = {}
for m, fn in modes.items():                       # warm-up: plan, capture, one replay
    for _ in range(2):
        finals[m] = fn()
    torch.cuda.synchronize()
for rnd in range(ROUNDS):                         # alternate the modes of this process
    for m, fn in modes.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(EDITS):
            fn()
        torch.cuda.synchronize()
        res["ms_per_edit"][m].append((time.perf_counter() - t0) * 1e3 / EDITS)
res["ms_per_step"] = {m: [v / STEPS for v in vs] for m, vs in res["ms_per_edit"].items()}
res["plan_keys"] = [str(k) for k in eng._plans]
res["launches"] = {str(k): dict(prologue=len(P.prologue), active=len(P.step_active), inactive=len(P.step_inactive)) for k, P in eng._plans.items()}
for m, x in finals.items():
    np.save(os.path.join(os.path.dirname(out_path), f"final_{tag}_{m}.npy"), x.cpu().numpy())
try:                                               # the FreeU launches of one active step, each between its own event pair
    for k, P in eng._plans.items():
        if "freeu" not in k:
            continue
        with torch.cuda.stream(eng.stream):
            P.step_idx.zero_()
        torch.cuda.synchronize()
        rows = []
        for _ in range(3):                         # (the first pass warms the caches; the last is reported)
            rows = [(meta["shape"], ms) for meta, ms in P.step_active.run_timed(eng.stream.cuda_stream) if meta["kind"] == "freeu"]
            with torch.cuda.stream(eng.stream):
                P.step_idx.zero_()
            torch.cuda.synchronize()
        res["freeu_launch_us"] = [dict(shape=list(s), us=round(ms * 1e3, 2)) for s, ms in rows]
except Exception as e:                             # noqa: BLE001  (optional detail: must not lose the timings)
    res["freeu_launch_us"] = {"error": f"{type(e).__name__}: {e}"[:300]}
json.dump(res, open(out_path, "w"))
print(json.dumps({k: res[k] for k in ("tag", "ms_per_step")}))
