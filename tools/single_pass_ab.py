#!/usr/bin/env python3
"""One process of the single-pass A/B at 512^2, batch 1 (the LCM row): run it from the root of a tree - the working tree, or
a worktree of the previous commit as tools/ab_prev.sh keeps one under _prev - and alternate the two on one box.

    python tools/single_pass_ab.py TAG OUT_JSON        TAG = prev (a tree without single-pass plans) | cur

prev: the 10-step DDIM edit with guidance_scale 1.0 on the duplicated plan (both CFG halves hold the positive prompt).  cur: the same
edit with single_pass=False and with single_pass=True, alternating, and a 4-step LCM single-pass edit.  Writes ms per edit and per step
of every round, the launch counts of every plan, the per-family time of one active step (launches run back to back, so the sum is
above the concurrent step time) and the final latents beside OUT_JSON."""
import json, os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
import torch
import bench
from blobctrl_amd.pipeline import BlobCtrlEngine
from blobctrl_amd.weights import PackedTrunk
from blobctrl_amd.splat import splat_features

tag, out_path = sys.argv[1], sys.argv[2]
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
pos = inp["prompt"][1:]
eng = BlobCtrlEngine(pw_u, pw_b, ucfg, bcfg, device=str(dev), scheduler="ddim")

def ddim(**kw):
    eng.set_scheduler("ddim")
    return eng.denoise(pos, inp["fg"], inp["bg"], score, inp["dino"], num_inference_steps=10, guidance_scale=1.0, latents=inp["latents"],
                       do_classifier_free_guidance=False, **kw)

modes = {"ddim_dup": lambda: ddim()} if tag == "prev" else {"ddim_dup": lambda: ddim(single_pass=False), "ddim_single": lambda: ddim(single_pass=True)}
steps = {"ddim_dup": 10, "ddim_single": 10, "lcm_single": 4}
if tag == "cur":
    from blobctrl_amd.schedulers import LCMScheduler, DDIMScheduler
    lcm = LCMScheduler.from_config(DDIMScheduler().config)
    noise = torch.randn(4, 1, 4, h, w, generator=torch.Generator().manual_seed(5)).to(dev)
    def lcm_edit():
        eng.set_scheduler(lcm.kind, lcm.table_params())
        return eng.denoise(pos, inp["fg"], inp["bg"], score, inp["dino"], num_inference_steps=4, guidance_scale=1.0, latents=inp["latents"],
                           do_classifier_free_guidance=False, variance_noise=noise)
    modes["lcm_single"] = lcm_edit
res = {"tag": tag, "ms_per_edit": {m: [] for m in modes}}
finals = {}
for m, fn in modes.items():                       # warm-up: plan, capture, two replays
    for _ in range(3):
        finals[m] = fn()
    torch.cuda.synchronize()
EDITS = 8
for rnd in range(4):                              # alternate the modes of this process
    for m, fn in modes.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(EDITS):
            fn()
        torch.cuda.synchronize()
        res["ms_per_edit"][m].append((time.perf_counter() - t0) * 1e3 / EDITS)
res["ms_per_step"] = {m: [v / steps[m] for v in vs] for m, vs in res["ms_per_edit"].items()}
res["plan_keys"] = [str(k) for k in eng._plans]
res["launches"] = {str(k): dict(prologue=len(P.prologue), active=len(P.step_active), inactive=len(P.step_inactive)) for k, P in eng._plans.items()}
for m, x in finals.items():
    np.save(os.path.join(os.path.dirname(out_path), f"final_{tag}_{m}.npy"), x.cpu().numpy())
try:                                               # per-family time of one active step, launches run one after another
    import collections
    res["families_ms"] = {}
    for k, P in eng._plans.items():
        fam = collections.defaultdict(float)
        with torch.cuda.stream(eng.stream):
            P.step_idx.zero_()                         # (a row of the table: the edits left the counter behind the last one)
        torch.cuda.synchronize()
        for meta, ms in P.step_active.run_timed(eng.stream.cuda_stream):
            fam[meta["kind"]] += ms
        res["families_ms"][str(k)] = {a: round(b, 4) for a, b in sorted(fam.items())}
    torch.cuda.synchronize()
except Exception as e:                             # noqa: BLE001  (optional detail: must not lose the timings)
    res["families_ms"] = {"error": f"{type(e).__name__}: {e}"[:300]}
json.dump(res, open(out_path, "w"))
print(json.dumps({k: res[k] for k in ("tag", "ms_per_edit")}))
