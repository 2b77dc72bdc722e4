#!/usr/bin/env python3
"""Compile the tiny-net edit of tests/golden/loop_tiny.npz (DDIM, 5 steps, guidance window [0, 1]) into a `.bcplan` file and write
its inputs / expected result as a flat binary for the plain-C host test (tests/c/plan_edit.c).  Runs WITHOUT a GPU: the plan is
compiled against host addresses and is relocatable.  Weights come from blobctrl_amd.synth (same seeds as every tiny fixture).

    <out>/tiny_edit.bcplan            plan: segments prologue / step_active / step_inactive, weights + scheduler tables embedded
    <out>/tiny_edit_io.bin            u32 count, then per record: char name[32], u64 bytes, data  (inputs named like the plan's
                                      buffers; "expected_latents" = the reference loop's final latents; "sequence" = int32 per step,
                                      1 = step_active)

`--eta ETA` compiles the stochastic-DDIM edit of tests/golden/loop_tiny_eta.npz instead (5 steps, window [0, 1], ETA must be that
run's eta): the plan then also holds the named buffer `variance_noise` [5][1][4][8][8] with the noise the reference drew embedded, and
"expected_latents" is that run's final latents.

`--euler TAG` compiles a case of tests/golden/loop_tiny_euler.npz instead (e.g. euler_leading_6: the Euler scheduler, whose plan
assembles its inputs with the `_scaled` entry points): "latents" is then the start noise times the table's init_noise_sigma, and
"expected_latents" that run's final latents - or the contents of `--expected FILE.npy` (e.g. what the in-process engine computed).

`--lcm TAG` compiles a case of tests/golden/loop_tiny_lcm.npz (e.g. lcm_nocfg_4: the LCM scheduler with guidance off, a single-pass plan
whose `ctx` holds the positive prompt only and whose steps end in bc_scheduler_step_single; the noise the reference drew is embedded).

`--requests` compiles the MIXED edit of a request batch of 3 instead (REQUESTS below: own step counts, guidance scales, control windows
and strengths per request; the Euler scheduler, so the inputs are assembled by the `_requests` entry points): a version-8 plan whose
steps end in bc_scheduler_step_requests.  The inputs are seeded request-batch tensors (`request_inputs`), "latents" holds every
request's start noise times its own init_noise_sigma, "expected_latents" is `--expected FILE.npy` (what the in-process engine computed).

`--stored-tables` writes tests/golden/plan_tables_before_setup_merge.json instead: per configuration of
tests/test_request_tables_cpu.py:stored_table_cases, the sha256 of every table `compile_plan` stores with its contents and the returned
segment list.  The committed file was written by the commit BEFORE `denoise` / `compile_plan` got their shared set-up; regenerating it
from later code makes the test that reads it vacuous.

`--gemm-records` writes tests/golden/gemm_records_before_resolve.json instead: per source of tests/gemm_records_common.py:sources (planner
cases, full-width plans, tiny-net plans, view problems), the count of launches and GEMMs and the sha256 of the canonical text of every
launch's `meta`, every `BcGemm` handed to bc_plan_add_gemm and the slab reserved per stream.  The committed file was written by the commit
BEFORE `Recorder.gemm` asked bc_gemm_resolve; regenerating it from later code makes the test that reads it vacuous.  `--gemm-records-text
NAME` prints the canonical text of one source instead (to diff a mismatch).

    python tools/make_plan_fixture.py [OUT_DIR] [--eta ETA | --euler TAG | --lcm TAG | --requests [--expected FILE.npy]]
    python tools/make_plan_fixture.py --stored-tables
    python tools/make_plan_fixture.py --gemm-records | --gemm-records-text NAME
"""
import argparse
import os
import struct
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from blobctrl_amd.pipeline import BlobCtrlEngine  # noqa: E402
from tests.common import TINY, g, tiny_weights  # noqa: E402
from tests.gpu_common import tiny_trunk_configs  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
# the mixed edit of `--requests`: one entry per request
REQUESTS = dict(num_inference_steps=[4, 6, 5], guidance_scale=[7.5, 3.0, 1.0], blobnet_control_guidance_start=[0.0, 0.2, 0.0],
                blobnet_control_guidance_end=[1.0, 0.7, 0.5], blobnet_conditioning_scale=[1.0, 0.0, 1.7])


def request_inputs(B=3, h=8, w=8, T=7):
    """The seeded request batch of `--requests` (every tensor with a leading B), as `BlobCtrlEngine.denoise` takes it."""
    return dict(prompt=g(32, 2 * B, T, TINY["ctx"]), fg=g(33, B, 4, h, w) * 0.18215 * 5, bg=g(34, B, 4, h, w) * 0.18215 * 5,
                score=g(36, B, 2, h, w).abs().clamp(max=1), dino=g(35, B, 1, TINY["feat"]), latents=g(31, B, 4, h, w))


def write_io(path, recs):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(recs)))
        for name, arr in recs.items():
            raw = np.ascontiguousarray(arr).tobytes()
            f.write(name.encode().ljust(32, b"\0"))
            f.write(struct.pack("<Q", len(raw)))
            f.write(raw)


def compile_requests(out, expected):
    """The `--requests` fixture: the mixed Euler edit of REQUESTS as a plan file + its inputs."""
    from blobctrl_amd import schedulers
    sched = schedulers.EulerDiscreteScheduler(steps_offset=1)
    usd, bsd = tiny_weights()
    ucfg, bcfg = tiny_trunk_configs()
    eng = BlobCtrlEngine(usd, bsd, ucfg, bcfg, device="cpu", scheduler="ddim", compile_only=True)
    eng.set_scheduler(sched.kind, sched.table_params())
    B, h, w, T = 3, 8, 8, 7
    seq = eng.compile_plan(os.path.join(out, "tiny_edit.bcplan"), B, h, w, T, TINY["ctx"], **REQUESTS)
    a = request_inputs(B, h, w, T)
    sigma0 = [eng._scheduler_table(n).init_noise_sigma for n in REQUESTS["num_inference_steps"]]
    feat16 = torch.zeros(B, 8, dtype=torch.float16)
    feat16[:, : TINY["feat"]] = a["dino"].reshape(B, -1).half()
    write_io(os.path.join(out, "tiny_edit_io.bin"), {
        "latents": torch.stack([a["latents"][b] * sigma0[b] for b in range(B)]).numpy(),
        "ctx": a["prompt"].half().numpy(), "fg_lat": a["fg"].numpy(), "bg_lat": a["bg"].numpy(),
        "bg_score": a["score"][:, 0].contiguous().numpy(), "fg_score": a["score"][:, 1].contiguous().numpy(),
        "feat": a["dino"].reshape(B, -1).numpy(), "feat16": feat16.numpy(),
        "expected_latents": (expected if expected is not None else np.zeros((B, 4, h, w))).astype(np.float32),
        "sequence": np.array([1 if s == "step_active" else 0 for s in seq], np.int32)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(REPO, "build", "plan_fixture"))
    ap.add_argument("--eta", type=float, default=0.0, help="stochastic DDIM: the eta of loop_tiny_eta.npz's 5-step run")
    ap.add_argument("--euler", default=None, help="a case of loop_tiny_euler.npz (Euler / Euler-ancestral / Heun)")
    ap.add_argument("--lcm", default=None, help="a case of loop_tiny_lcm.npz (LCM with or without guidance, single-pass DDIM / UniPC)")
    ap.add_argument("--requests", action="store_true", help="the mixed edit of a request batch of 3 (REQUESTS), Euler")
    ap.add_argument("--expected", default=None, help=".npy file with the expected final latents (default: the reference loop's)")
    ap.add_argument("--stored-tables", action="store_true", help="write tests/golden/plan_tables_before_setup_merge.json")
    ap.add_argument("--gemm-records", action="store_true", help="write tests/golden/gemm_records_before_resolve.json")
    ap.add_argument("--gemm-records-text", default=None, metavar="NAME", help="print the canonical text of one source of --gemm-records")
    args = ap.parse_args()
    if args.gemm_records or args.gemm_records_text:
        import json
        from tests.gemm_records_common import sources
        if args.gemm_records_text:
            sys.stdout.write(dict(sources())[args.gemm_records_text]().text())
            return
        records = {}
        for name, record in sources():
            records[name] = record().entry()
            print(name, records[name], flush=True)
        with open(os.path.join(GOLD, "gemm_records_before_resolve.json"), "w") as f:
            json.dump(records, f, indent=0, sort_keys=True)
            f.write("\n")
        print("gemm_records_before_resolve.json:", len(records), "sources,", sum(r["gemms"] for r in records.values()), "GEMMs")
        return
    if args.stored_tables:
        import json
        import tempfile
        from tests.test_request_tables_cpu import stored_tables
        with tempfile.TemporaryDirectory() as tmp:
            tables = stored_tables(tmp)
        with open(os.path.join(GOLD, "plan_tables_before_setup_merge.json"), "w") as f:
            json.dump(tables, f, indent=1, sort_keys=True)
            f.write("\n")
        print("plan_tables_before_setup_merge.json:", len(tables), "configurations")
        return
    OUT = args.out
    os.makedirs(OUT, exist_ok=True)
    if args.requests:
        compile_requests(OUT, np.load(args.expected) if args.expected else None)
        for fn in ("tiny_edit.bcplan", "tiny_edit_io.bin"):
            print(fn, os.path.getsize(os.path.join(OUT, fn)), "bytes")
        return
    z = np.load(os.path.join(GOLD, "loop_tiny.npz"))
    extra, expected = {}, z["ddim_5_final"]
    sigma0, steps, window, sched = 1.0, 5, (0.0, 1.0), None
    if args.euler:
        import json
        from blobctrl_amd import schedulers
        ze = np.load(os.path.join(GOLD, "loop_tiny_euler.npz"))
        kw = json.loads(str(ze[f"{args.euler}_kw"]))
        cls, steps, ts = kw.pop("cls"), kw.pop("n"), kw.pop("timesteps")
        sched = {"euler": schedulers.EulerDiscreteScheduler, "euler_ancestral": schedulers.EulerAncestralDiscreteScheduler,
                 "heun": schedulers.HeunDiscreteScheduler}[cls](steps_offset=1, **kw)
        sched.set_timesteps(timesteps=ts) if ts is not None else sched.set_timesteps(steps)
        sigma0, window, expected = sched.init_noise_sigma, tuple(float(v) for v in ze[f"{args.euler}_window"]), ze[f"{args.euler}_final"]
        if ts is not None:
            extra = dict(timesteps=ts)
        if f"{args.euler}_noise" in ze.files:
            extra["variance_noise"] = torch.from_numpy(ze[f"{args.euler}_noise"])
    guidance, positive_only = 7.5, False
    if args.lcm:
        import json
        from blobctrl_amd import schedulers
        zl = np.load(os.path.join(GOLD, "loop_tiny_lcm.npz"))
        kw = json.loads(str(zl[f"{args.lcm}_kw"]))
        src = schedulers.DDIMScheduler().config
        sched = {"lcm": schedulers.LCMScheduler, "ddim": schedulers.DDIMScheduler, "unipc": schedulers.UniPCMultistepScheduler}[kw["cls"]].from_config(src)
        sched.set_timesteps(**kw["set_timesteps"])
        steps, guidance = len(sched.timesteps), float(kw["guidance_scale"])
        window, expected = tuple(float(v) for v in zl[f"{args.lcm}_window"]), zl[f"{args.lcm}_final"]
        positive_only = guidance <= 1.0
        if positive_only:
            extra["single_pass"] = True
        if f"{args.lcm}_noise" in zl.files:                                # n - 1 draws; the last step's slice is never read
            noise = torch.from_numpy(zl[f"{args.lcm}_noise"])
            extra["variance_noise"] = torch.cat([noise, torch.zeros_like(noise[:1])], 0)
    if args.expected:
        expected = np.load(args.expected)
    if args.eta:
        ze = np.load(os.path.join(GOLD, "loop_tiny_eta.npz"))
        if float(ze["ddim_5_eta"]) != args.eta:
            sys.exit(f"--eta {args.eta}: the 5-step run of loop_tiny_eta.npz was drawn with eta = {float(ze['ddim_5_eta'])}")
        extra = dict(eta=args.eta, variance_noise=torch.from_numpy(ze["ddim_5_noise"]))
        expected = ze["ddim_5_final"]
    usd, bsd = tiny_weights()
    ucfg, bcfg = tiny_trunk_configs()
    eng = BlobCtrlEngine(usd, bsd, ucfg, bcfg, device="cpu", scheduler="ddim", compile_only=True)
    if sched is not None:
        eng.set_scheduler(sched.kind, sched.table_params())
    B, h, w, T = 1, 8, 8, 7
    seq = eng.compile_plan(os.path.join(OUT, "tiny_edit.bcplan"), B, h, w, T, TINY["ctx"], steps, guidance_scale=guidance,
                           blobnet_conditioning_scale=1.0, blobnet_control_guidance_start=window[0], blobnet_control_guidance_end=window[1],
                           **extra)
    score = torch.from_numpy(z["gs_score"]).float()                     # [1,2,h,w] = (bg, fg)
    dino = g(35, 1, 1, TINY["feat"])
    feat16 = torch.zeros(1, 8, dtype=torch.float16)
    feat16[:, : TINY["feat"]] = dino.reshape(1, -1).half()
    recs = {
        "latents": (g(31, B, 4, h, w) * sigma0).numpy(),                   # x init_noise_sigma (= 1 for DDIM)
        "ctx": g(32, 2 * B, T, TINY["ctx"])[B if positive_only else 0:].half().numpy(),     # a single-pass plan: the positive prompt only
        "fg_lat": (g(33, 1, 4, h, w) * 0.18215 * 5).numpy(),
        "bg_lat": (g(34, 1, 4, h, w) * 0.18215 * 5).numpy(),
        "bg_score": score[:, 0].contiguous().numpy(),
        "fg_score": score[:, 1].contiguous().numpy(),
        "feat": dino.reshape(1, -1).numpy(),
        "feat16": feat16.numpy(),
        "expected_latents": expected.astype(np.float32),
        "sequence": np.array([1 if s == "step_active" else 0 for s in seq], np.int32),
    }
    write_io(os.path.join(OUT, "tiny_edit_io.bin"), recs)
    for fn in ("tiny_edit.bcplan", "tiny_edit_io.bin"):
        print(fn, os.path.getsize(os.path.join(OUT, fn)), "bytes")


if __name__ == "__main__":
    main()
