#!/usr/bin/env python3
"""Benchmark of the BlobCtrl denoising hot path on MI355X (contract: see the task statement / DESIGN.md section 6).

One bench "step" = ONE complete 512x512 edit of BASELINE.json configs[1]: batch 1, 50 scheduler steps, each step =
BlobNet (batch 1) + patched UNet (CFG batch 2) + crop/CFG/scheduler update, hipGraph-replayed, inputs resident in HBM.
metric = edits/s over all ranks (weak scaling: every rank runs its own K edits, no data-path collective).
A plain run times only that: set-up, warm-up, the timed edits, the result line.  `--full` adds the optional blocks: `roofline` for
the dominant kernel (HIP-event timed on the launch stream), `cpu_baseline` (the CPU oracle, one denoise step of the same workload on
the host cores, rank 0 / N=1 only), `box_calibration`, the other configurations and the end-to-end timings.  `--dump-outputs DIR`
writes what the last timed edit returned (rank 0) as DIR/latents.npy.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

import torch  # noqa: E402

MFMA_PEAK_TFLOPS = 2500.0      # dense fp16/bf16 MFMA peak, MI355X_MICROARCH.md "Chip-level parameters"


def full_configs():
    from blobctrl_amd.engine import TrunkConfig
    u = TrunkConfig(in_channels=5, block_out_channels=(320, 640, 1280, 1280), num_heads=8, norm_num_groups=32,
                    cross_attention_dim=768, out_channels=4, is_blobnet=False)
    b = TrunkConfig(in_channels=1029, block_out_channels=(320, 640, 1280, 1280), num_heads=8, norm_num_groups=32,
                    cross_attention_dim=None, out_channels=0, is_blobnet=True)
    return u, b


def synth_weights():
    from blobctrl_amd import synth
    us = synth.trunk_param_shapes(5, (320, 640, 1280, 1280), 2, 768, 4, blobnet=False)
    bs = synth.trunk_param_shapes(1029, (320, 640, 1280, 1280), 2, None, None, blobnet=True)
    return synth.synth_state_dict(us, 1234), synth.synth_state_dict(bs, 1235)


def synth_inputs(h, w, T=77, ctx=768, feat=1024, batch=1):
    """SURVEY 8d synthetic inputs: seeded latents / prompt embeddings / DINO vector, move_hat blob scaled to the canvas."""
    import numpy as np
    from blobctrl_amd.splat import blob_dict_from_ellipse

    def g(seed, *shape):
        return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(shape).astype(np.float32))
    s = (8 * w) / 512.0
    ell = [[361.1067 * s, 367.8526 * s], [85.4812 * s, 103.6543 * s], 87.3739]
    return dict(fg=g(1, 1, 4, h, w) * 0.18215 * 5, bg=g(2, 1, 4, h, w) * 0.18215 * 5, prompt=g(3, 2 * batch, T, ctx),
                dino=g(4, 1, 1, feat), latents=g(1248464818 % (2 ** 31), batch, 4, h, w),
                blob=blob_dict_from_ellipse(ell, 8 * w, 8 * h))


def cpu_baseline_worker(h, w, steps):
    """`bench.py --cpu-baseline-worker`: the CPU oracle (oracle/, kind 'port') timed on the host cores in a process of its own, which
    never touches the GPU.  FULL denoise steps of the same workload as the reference executes them (BlobNet AND UNet at CFG batch 2,
    fp32, pipe:1043-1090).  The process pins itself to the cores of ONE socket before the first torch operation (the OpenMP pool
    inherits the mask; on the two-socket hosts an unpinned 32-thread run measured 28 s per step, the real reference does 18.7 s on
    8 cores), then takes one warm-up step and one step at each candidate thread count {8, 16, 32, 64} that the socket can hold; the
    reported step time is the best candidate's.  The 50-step edit is an extrapolation of that step and is labelled as such."""
    sock = socket0_cpus()
    try:
        avail = sorted(os.sched_getaffinity(0))
    except AttributeError:
        avail = list(range(os.cpu_count() or 1))
    cpus = [c for c in sock if c in avail] or avail
    pinned = False
    try:
        os.sched_setaffinity(0, cpus)
        pinned = True
    except (AttributeError, OSError):
        pass
    from oracle import blob_splat
    from oracle.nets import NetConfig
    from oracle.pipeline import noise_pred_step
    usd, bsd = synth_weights()
    inp = synth_inputs(h, w)
    physical = physical_cores() or len(avail)
    ucfg = NetConfig(in_channels=5, cross_attention_dim=768)
    bcfg = NetConfig(in_channels=1029, cross_attention_dim=None)
    b = inp["blob"]
    score = torch.from_numpy(blob_splat.splat_scores(float(b["xs"]), float(b["ys"]), b["covs"][0, 0].numpy(), 1.0, h, w)).float()
    B2 = 2
    fg, bg = inp["fg"].repeat(B2, 1, 1, 1), inp["bg"].repeat(B2, 1, 1, 1)
    bg_s, fg_s = score.unbind(dim=1)
    bg_s, fg_s = bg_s.unsqueeze(1).repeat(B2, 1, 1, 1), fg_s.unsqueeze(1).repeat(B2, 1, 1, 1)
    feats = torch.einsum("nmhw,nmc->nchw", fg_s, inp["dino"].repeat(B2, 1, 1)).contiguous()

    def one_step(t):
        """pipe:1031-1098: BlobNet on the CFG batch, right-square slices of its residuals into the UNet, crop + CFG."""
        return noise_pred_step(usd, ucfg, bsd, bcfg, inp["latents"], t, inp["prompt"], fg, bg, fg_s, bg_s, feats, 1.0, 7.5)

    # the parent's timed GPU region comes first: its host thread feeds the whole-edit graph to the queues for the length of an edit and must
    # not compete with this process's OpenMP pool; the parent creates the "go" file when its headline timing is done
    go = os.environ.get("BC_CPU_BASELINE_GO")
    t_wait = time.perf_counter()
    parent = os.getppid()
    while go and not os.path.exists(go) and time.perf_counter() - t_wait < 900:
        if os.getppid() != parent:                     # the bench process is gone: nobody will read the result
            return
        time.sleep(0.2)
    cands = sorted({min(len(cpus), n) for n in (8, 16, 32, 64)})
    budget_s = float(os.environ.get("BC_CPU_BASELINE_BUDGET_S", "150"))
    t_begin = time.perf_counter()
    table = []
    with torch.no_grad():
        torch.set_num_threads(cands[min(1, len(cands) - 1)])
        t0 = time.perf_counter()
        one_step(torch.tensor(999))                      # warm-up step (primitive creation, first touch): not used
        table.append(["warm-up", round(time.perf_counter() - t0, 3)])
        per = {}
        for k, nt in enumerate(cands):
            if per and time.perf_counter() - t_begin + min(per.values()) > budget_s:
                break                                    # (the bench must finish in minutes: remaining candidates are skipped, and listed)
            torch.set_num_threads(nt)
            t0 = time.perf_counter()
            one_step(torch.tensor(979 - 20 * k))
            per[nt] = time.perf_counter() - t0
            table.append([nt, round(per[nt], 3)])
    cores = min(per, key=per.get)
    t_step = per[cores]
    skipped = [n for n in cands if n not in per]
    sample = (f"one full denoise step (BlobNet + UNet at CFG batch 2 as the reference executes them, fp32, {8*h}x{8*w}) per candidate "
              f"thread count after one warm-up step, in a separate process {'pinned to the ' + str(len(cpus)) + ' CPUs of socket 0' if pinned else 'not pinned'}: "
              f"{{{', '.join(f'{k}: {v:.1f} s' for k, v in sorted(per.items()))}}}"
              f"{' (skipped for the time budget: ' + str(skipped) + ')' if skipped else ''}; best {t_step:.2f} s/step on {cores} threads "
              f"({physical} physical cores on the host); value = 1 / (s/step x {steps}) is an EXTRAPOLATION of the measured step time "
              "to the whole edit (the scheduler update is negligible)")
    ratio = None
    try:                  # the port against the REAL reference on the build container's cores (tools/make_golden.py golden_cpu_step_seconds)
        with open(os.path.join(REPO, "tests", "golden", "cpu_step_seconds.json")) as f:
            ref = json.load(f)
        ratio = dict(port_vs_reference_ratio=ref["port_vs_reference_ratio"], reference_s_per_step=ref["reference_s"], port_s_per_step=ref["port_s"],
                     measured_on=f"{ref['threads']} threads of the build container, same weights and inputs, interleaved")
    except (OSError, KeyError, ValueError):
        pass
    print(json.dumps(dict(value=1.0 / (t_step * steps), unit="edits/s", cores=cores, kind="port", sample=sample, port_vs_reference=ratio,
                          host_cpus_visible=len(avail), physical_cores=physical, pinned_cpus=len(cpus) if pinned else None,
                          s_per_step=round(t_step, 3), step_times_s=table,
                          c1_20step_edit_s_extrapolated=round(t_step * 20, 1), edit_s_extrapolated=round(t_step * steps, 1))), flush=True)


def socket0_cpus():
    """Logical CPUs of physical package 0 (/proc/cpuinfo), hyper-thread siblings included; [] when unknown."""
    try:
        cpus, cur, phys = [], None, None
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.startswith("processor"):
                    cur = int(ln.split(":")[1])
                elif ln.startswith("physical id"):
                    phys = ln.split(":")[1].strip()
                elif not ln.strip():
                    if cur is not None and phys in (None, "0"):
                        cpus.append(cur)
                    cur = phys = None
        return cpus
    except OSError:
        return []


def start_cpu_baseline(h, w, steps):
    """Start the CPU-baseline worker as a child of THIS process, which has made no GPU call yet (a GPU-initialised process must not be
    the parent of an exec on this pool).  It runs beside the GPU benchmark on its own socket's cores; `collect_cpu_baseline` waits."""
    import subprocess
    import tempfile
    out = tempfile.NamedTemporaryFile("w+", suffix=".json", delete=False)
    go = out.name + ".go"
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", BC_CPU_BASELINE_GO=go)       # (the worker never sees a GPU)
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--cpu-baseline-worker", "--res", str(8 * h), "--denoise-steps", str(steps)],
                         stdout=out, stderr=subprocess.DEVNULL, env=env)
    return p, out, go


def release_cpu_baseline(handle):
    """The headline timing is done: let the worker start its measured steps (it has generated its weights meanwhile)."""
    if handle is not None:
        open(handle[2], "w").close()


def collect_cpu_baseline(handle, timeout_s=600):
    p, out, go = handle
    try:
        p.wait(timeout=timeout_s)
    except Exception:
        p.kill()
        return dict(error=f"cpu-baseline worker did not finish within {timeout_s} s")
    out.seek(0)
    lines = [ln for ln in out.read().splitlines() if ln.startswith("{")]
    for fn in (out.name, go):
        try:
            os.unlink(fn)
        except OSError:
            pass
    if p.returncode or not lines:
        return dict(error=f"cpu-baseline worker failed (exit code {p.returncode})")
    return json.loads(lines[-1])


def physical_cores():
    """Distinct (physical id, core id) pairs of /proc/cpuinfo, restricted to nothing (the affinity mask caps the choice separately)."""
    try:
        seen, phys, core = set(), None, None
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.startswith("physical id"):
                    phys = ln.split(":")[1].strip()
                elif ln.startswith("core id"):
                    core = ln.split(":")[1].strip()
                elif not ln.strip():
                    if phys is not None and core is not None:
                        seen.add((phys, core))
                    phys = core = None
        return len(seen)
    except OSError:
        return 0


def make_request_batch(ids, h, w, dev):
    """BASELINE configs[2] / [3]: `ids` independent edit requests as ONE per-request batch (own fg / bg latents, ellipse,
    DINO vector, prompt, noise; every 4th request is a `remove`: strength 0.0 and gs_score = (bg 1, fg 0), inf:175-188)."""
    import numpy as np
    from blobctrl_amd.splat import blob_dict_from_ellipse, splat_features
    gen = lambda seed, *shape: torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(shape).astype(np.float32))
    fg, bg, sc, dino, lat, neg, pos, strength = [], [], [], [], [], [], [], []
    for i in ids:
        sx = (8 * w) / 512.0
        ell = [[(200.0 + 23.0 * (i % 9)) * sx, (180.0 + 31.0 * (i % 7)) * sx], [(60.0 + 5.0 * (i % 11)) * sx, (90.0 + 3.0 * (i % 13)) * sx],
               float((17 * i) % 180)]
        sco = splat_features(**blob_dict_from_ellipse(ell, 8 * w, 8 * h), score_size=(h, w), return_d_score=True, device=str(dev))
        remove = i % 4 == 1
        if remove:
            sco = torch.stack([torch.ones_like(sco[:, 0]), torch.zeros_like(sco[:, 1])], 1)
        sc.append(sco)
        strength.append(0.0 if remove else 1.0)
        fg.append(gen(10_000 + i, 1, 4, h, w) * 0.18215 * 5)
        bg.append(gen(20_000 + i, 1, 4, h, w) * 0.18215 * 5)
        dino.append(gen(30_000 + i, 1, 1, 1024))
        lat.append(gen(40_000 + i, 1, 4, h, w))
        neg.append(gen(50_000, 1, 77, 768))
        pos.append(gen(60_000 + i, 1, 77, 768))
    cat = lambda xs: torch.cat(xs, 0).to(dev)
    return dict(prompt=cat(neg + pos), fg=cat(fg), bg=cat(bg), score=torch.cat(sc, 0), dino=cat(dino), latents=cat(lat),
                strength=strength)


def other_configs(pipe, pw_u, pw_b, ucfg, bcfg, dev, denoise_steps, scheduler):
    """The other BASELINE configurations on the driver's clock, 1 warm-up + 2 timed edits each, inputs
    resident in HBM, same engine and packed weights as the headline run:
      c3  configs[2]: batch 8, MIXED operations (per-request inputs and strengths, two `remove`), 512^2, hipGraph-captured loop
      c5  configs[4]: 768^2, batch 4
      unipc: the headline workload with the scheduler the reference scripts run (inf:276)."""
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from blobctrl_amd.splat import splat_features
    out = {}

    def timed(fn, edits=2):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(edits):
            o = fn()
        torch.cuda.synchronize()
        assert torch.isfinite(o).all()
        return (time.perf_counter() - t0) / edits

    # (the other scheduler FIRST: behind the C3 / C5 blocks - five seconds of full-chip load - the same two edits read up to 10 % slower)
    other = "unipc" if scheduler == "ddim" else "ddim"
    eng = BlobCtrlEngine(pw_u, pw_b, ucfg, bcfg, device=str(dev), scheduler=other)
    i1 = synth_inputs(64, 64)
    d1 = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in i1.items()}
    s1 = splat_features(**i1["blob"], score_size=(64, 64), return_d_score=True, device=str(dev))
    dt = timed(lambda: eng(d1["prompt"], d1["fg"], d1["bg"], s1, d1["dino"], num_inference_steps=denoise_steps, guidance_scale=7.5,
                           latents=d1["latents"], blobnet_conditioning_scale=1.0))
    out[f"{other}_ms_per_step"] = round(dt / denoise_steps * 1e3, 3)
    rb = make_request_batch(list(range(8)), 64, 64, dev)
    dt = timed(lambda: pipe(rb["prompt"], rb["fg"], rb["bg"], rb["score"], rb["dino"], num_inference_steps=denoise_steps, guidance_scale=7.5,
                            latents=rb["latents"], blobnet_conditioning_scale=rb["strength"]))
    out["c3_batch8_mixed_ms_per_step"] = round(dt / denoise_steps * 1e3, 3)
    out["c3_batch8_mixed_images_per_s"] = round(8 / dt, 4)
    fl3 = pipe.plan_for(8, 64, 64, 77, 768, denoise_steps, per_request=True).step_active.flops
    out["c3_frac_of_peak"] = round(fl3 * denoise_steps / dt / 1e12 / MFMA_PEAK_TFLOPS, 4)
    h5 = 96
    i5 = synth_inputs(h5, h5, batch=4)
    d5 = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in i5.items()}
    s5 = splat_features(**i5["blob"], score_size=(h5, h5), return_d_score=True, device=str(dev))
    dt = timed(lambda: pipe(d5["prompt"], d5["fg"], d5["bg"], s5, d5["dino"], num_inference_steps=denoise_steps, guidance_scale=7.5,
                            latents=d5["latents"], blobnet_conditioning_scale=1.0))
    out["c5_768_batch4_ms_per_step"] = round(dt / denoise_steps * 1e3, 3)
    out["c5_768_batch4_images_per_s"] = round(4 / dt, 4)
    fl5 = pipe.plan_for(4, h5, h5, 77, 768, denoise_steps).step_active.flops
    out["c5_frac_of_peak"] = round(fl5 * denoise_steps / dt / 1e12 / MFMA_PEAK_TFLOPS, 4)
    out["note"] = (f"1 warm-up + 2 timed edits each, {denoise_steps} steps, guidance window [0,1], CFG 7.5; c3 / c5 with the "
                   f"{scheduler.upper()} scheduler of the headline run; ms per denoise step of the WHOLE batch")
    return out


def plan_variants(plan):
    """Launches per kernel instantiation (rocprofv3 names) of one BlobNet-active step of the plan."""
    import collections
    c = collections.Counter((m.get("rocprof") or m.get("variant") or m["kind"]) for m in plan.step_active.meta if m["kind"] not in ("event_record", "event_wait"))
    return dict(sorted(c.items(), key=lambda kv: -kv[1]))


def metric_name(args):
    """The headline metric name is reserved for the headline workload (512^2, batch 1, 50 steps, --steps edits per rank); anything
    else carries its parameters in the name so that it is never filed under the headline."""
    name = f"{args.res}x{args.res}_{args.denoise_steps}step_blobctrl_edits_per_sec"
    if args.batch != 1:
        name += f"_batch{args.batch}"
    if args.requests:
        name += f"_requests{args.requests}"
    return name


def device_identity(dev):
    """(local device index, PCI bus id, uuid when the runtime exposes one) of this rank's GPU: the bench line proves N distinct devices."""
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    props = torch.cuda.get_device_properties(idx)
    bdf = None
    try:
        bdf = f"{props.pci_domain_id:04x}:{props.pci_bus_id:02x}:{props.pci_device_id:02x}"
    except AttributeError:
        pass
    return dict(local_device=idx, pci_bdf=bdf, uuid=str(getattr(props, "uuid", "")) or None, name=props.name)


def csrc_sha():
    """Hash of the kernel sources: identifies the build a committed PMC summary was measured on."""
    import hashlib
    hsh = hashlib.sha1()
    d = os.path.join(REPO, "blobctrl_amd", "csrc")
    for f in sorted(x for x in os.listdir(d) if x.endswith((".hip", ".h"))):
        with open(os.path.join(d, f), "rb") as fh:
            hsh.update(f.encode() + b"\0" + fh.read())
    return hsh.hexdigest()[:12]


def _profile_doc(pattern, res, batch):
    """The committed PMC summary (profiles/<round>_<pattern>) taken on exactly these kernel sources at the headline shape, or (None, why)."""
    import glob
    files = sorted(glob.glob(os.path.join(REPO, "profiles", "*" + pattern)))      # by name (r1_, r2_, ...), never by mtime
    if not files:
        return None, f"no profiles/*{pattern}"
    docs = []
    for fn in files:
        with open(fn) as f:
            docs.append((fn, json.load(f)))
    # (round 6: summaries exist for several workloads - r6_c3_* batch 8, r6_c5_* 768^2 batch 4, r6_b2_* batch 2; a summary states its own)
    docs = [fd for fd in docs if (fd[1].get("res", 512), fd[1].get("batch", 1)) == (res, batch)]
    if not docs:
        return None, f"no profiles/*{pattern} measured at {res}x{res} batch {batch}"
    match = [fd for fd in docs if fd[1].get("csrc_sha") == csrc_sha()]
    fn, doc = (match or docs)[-1]                      # the summary measured on THESE kernel sources, else the newest round's (refused below)
    name = os.path.relpath(fn, REPO)
    if doc.get("csrc_sha") != csrc_sha():
        return None, f"{name} was measured on kernel sources {doc.get('csrc_sha', '(unrecorded)')}, this run is {csrc_sha()}"
    return (name, doc), None


def _rows_of(doc, rocprof_name):
    """Rows of a PMC summary for ONE kernel instantiation, by the name rocprofv3 prints (e.g. `conv_wreg_kernel<2>`)."""
    return [r for r in doc["kernels"] if rocprof_name + "(" in r["kernel"].replace("(anonymous namespace)::", "")]


def pmc_traffic(rocprof_name, res, batch):
    """HBM bytes per launch of the dominant kernel.  PMC counters cannot be read from inside the timed process: the figure comes
    from the committed rocprofv3 summary of this same command (tools/profile_round.sh: separate --pmc FETCH_SIZE and --pmc
    WRITE_SIZE passes, gfx950 correction 2*FETCH + WRITE).  It is reported ONLY when that summary was taken on exactly these
    kernel sources (csrc hash) at the headline shape; otherwise `traffic` is null and `traffic_source` says why.  The average is over
    exactly the launches of the instantiation the bench bucket holds (the bucket IS that instantiation)."""
    hit, why = _profile_doc("pmc_hbm_traffic.json", res, batch)
    if hit is None:
        return None, why, None
    name, doc = hit
    rows = _rows_of(doc, rocprof_name)
    n = sum(r["launches"] for r in rows)
    if not n:
        return None, f"{name} has no row for {rocprof_name}", None
    steps_prof = doc.get("denoise_steps_profiled")
    ours = [r for r in doc["kernels"] if "anonymous namespace" in r["kernel"] or "_GLOBAL__N_" in r["kernel"]]      # (this library's kernels)
    step_gb = round(sum(r["hbm_bytes_per_launch_corrected"] * r["launches"] for r in ours) / steps_prof / 1e9, 2) if steps_prof else None
    return int(sum(r["hbm_bytes_per_launch_corrected"] * r["launches"] for r in rows) / n), \
        f"{name} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command on kernel sources {doc['csrc_sha']}; 2*FETCH+WRITE)", step_gb


def pmc_mfma_busy(rocprof_name, res, batch):
    """MFMA-pipe busy fraction of the dominant kernel from the committed SQ-counter pass (same rules as pmc_traffic)."""
    hit, why = _profile_doc("pmc_mfma_util_per_kernel.json", res, batch)
    if hit is None:
        return None
    rows = _rows_of(hit[1], rocprof_name)
    n = sum(r["launches"] for r in rows)
    return round(sum(r["mfma_busy_frac"] * r["launches"] for r in rows) / n, 4) if n else None


def roofline(pipe, plan, res=512, batch=1):
    """HIP-event time every launch of one BlobNet-active step on the launch stream; report the dominant kernel."""
    s = pipe.stream.cuda_stream
    with torch.cuda.stream(pipe.stream):
        plan.step_idx.zero_()
    plan.step_active.run(s)                      # warm
    with torch.cuda.stream(pipe.stream):
        plan.step_idx.zero_()
    # serial eager replay of the launch list, HIP events around every launch on the launch stream; a split-K GEMM is divided at an
    # event between its main kernel and its reducer, so that every bucket below is ONE kernel, as rocprofv3 reports it
    timed = []
    for m, ms_main, ms_red in plan.step_active.run_timed_kernels(s):
        # (a bucket = ONE kernel instantiation, named as rocprofv3 names it: the rows of profiles/*kernel_stats*.csv)
        timed.append((dict(m, variant=m.get("rocprof") or (m["variant"] or "").replace("+splitk_reduce", "")), ms_main))
        if ms_red > 0:
            timed.append((dict(kind="splitk_reduce", variant="splitk_reduce_vec_kernel", flops=0, bytes=0, shape=m["shape"]), ms_red))
    pipe.stream.synchronize()
    by = {}
    for m, ms in timed:
        v = m["variant"] or m["kind"]
        a = by.setdefault(v, dict(ms=0.0, flops=0, n=0, bytes=0))
        a["ms"] += ms
        a["flops"] += m["flops"]
        a["bytes"] += m.get("bytes", 0)
        a["n"] += 1
    total_ms = sum(a["ms"] for a in by.values())
    shapes = {}
    for m, ms in timed:
        key = (m["kind"], m["variant"], m["shape"])
        a = shapes.setdefault(key, dict(ms=0.0, n=0, flops=0, bytes=0))
        a["ms"] += ms
        a["n"] += 1
        a["flops"] += m["flops"]
        a["bytes"] += m.get("bytes", 0)
    detail = [dict(kind=k[0], variant=k[1], shape=k[2], launches=v["n"], ms=round(v["ms"], 4),
                   tflops=round(v["flops"] / max(v["ms"], 1e-9) / 1e9, 1), gbps=round(v["bytes"] / max(v["ms"], 1e-9) / 1e6, 1))
              for k, v in sorted(shapes.items(), key=lambda kv: -kv[1]["ms"])][:60]
    # Dominance is decided on kernel time, not on launch count: an event pair around a launch also measures a fixed launch /
    # event overhead (calibrated below on a 64-element kernel), which would favour buckets of many small launches over the
    # rocprofv3 ranking (profiles/*kernel_stats*.csv).  The reported duration of the chosen kernel stays the raw event time.
    import ctypes as C
    from blobctrl_amd import _lib
    lib = _lib.load()
    tiny = torch.zeros(64, dtype=torch.float16, device=pipe.device)
    ovh = []
    for _ in range(12):
        a_, b_ = C.c_void_p(), C.c_void_p()
        lib.bc_event_create(C.byref(a_)); lib.bc_event_create(C.byref(b_))
        lib.bc_event_record(a_, s)
        lib.bc_silu(tiny.data_ptr(), tiny.data_ptr(), 64, s)
        lib.bc_event_record(b_, s)
        pipe.stream.synchronize()
        ms_ = C.c_float()
        lib.bc_event_elapsed_ms(a_, b_, C.byref(ms_))
        ovh.append(ms_.value)
        lib.bc_event_destroy(a_); lib.bc_event_destroy(b_)
    overhead_ms = sorted(ovh)[len(ovh) // 2]
    cand = {k: a for k, a in by.items() if a["flops"] > 0}
    dom = max(cand, key=lambda k: cand[k]["ms"] - cand[k]["n"] * overhead_ms)
    a = cand[dom]
    achieved = a["flops"] / (a["ms"] * 1e-3) / 1e12
    table = {k: dict(launches=v["n"], ms=round(v["ms"], 4), tflops=round(v["flops"] / max(v["ms"], 1e-9) / 1e9, 1),
                     gbps=round(v["bytes"] / max(v["ms"], 1e-9) / 1e6, 1))
             for k, v in sorted(by.items(), key=lambda kv: -kv[1]["ms"])}
    traffic, traffic_source, step_traffic_gb = pmc_traffic(dom, res, batch)
    # algorithmic HBM bytes per launch of the dominant kernel (operands once: activation + weights + fp16 result), to read `traffic` against:
    # over exactly the launches of the bucket (= the instantiation the PMC rows hold)
    alg = [m["bytes"] for m, _ in timed if (m["variant"] or m["kind"]) == dom and m.get("bytes")]
    step_alg_gb = round(sum(m.get("bytes", 0) for m, _ in timed) / 1e9, 2)
    # The same figure over the launches of that kernel whose grid fills the chip (>= one workgroup per CU).  The plan deliberately leaves
    # some passes half-filled (the other trunk's kernels run beside them: DESIGN 3.7); alone in this serial replay such a launch shows
    # half the throughput, which says nothing about the kernel.  `frac` above is over ALL its launches, as they are shipped.
    full_grid = None
    if dom.startswith("conv_wreg_kernel") or dom.startswith("conv_halo_kernel"):
        fl = fms = fn = 0
        for m, ms in timed:
            if (m["variant"] or m["kind"]).split("<")[0] == dom.split("<")[0] and m.get("shape") and len(m["shape"]) >= 5:
                _, M_, N_, _, sk_ = m["shape"][:5]
                if -(-M_ // 128) * (N_ // 160) * sk_ >= 256:
                    fl, fms, fn = fl + m["flops"], fms + ms, fn + 1
        if fn:
            full_grid = dict(launches=fn, avg_launch_us=round(fms * 1e3 / fn, 2), achieved=round(fl / (fms * 1e-3) / 1e12, 2),
                             frac=round(fl / (fms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4))
    return dict(bound="mfma", kernel=dom, achieved=round(achieved, 2), peak=MFMA_PEAK_TFLOPS, unit="TFLOP/s",
                frac=round(achieved / MFMA_PEAK_TFLOPS, 4), full_grid_launches=full_grid, traffic=traffic, traffic_source=traffic_source,
                algorithmic_bytes_per_launch=int(sum(alg) / len(alg)) if alg else None, mfma_busy=pmc_mfma_busy(dom, res, batch),
                step_traffic_gb=step_traffic_gb, step_algorithmic_gb=step_alg_gb, launches_per_step=a["n"],
                avg_launch_us=round(a["ms"] * 1e3 / a["n"], 2), flops_per_launch=a["flops"] / a["n"],
                step_ms_event_sum=round(total_ms, 3), event_overhead_us=round(overhead_ms * 1e3, 2)), \
        dict(by_kernel=table, top_shapes=detail)


# Reference readings of the two calibration probes (the box the round-6 profiles and parity margins were taken on): a box's speed index is the mean
# of its two ratios to these
CAL_REF = {"gemm_8192_tflops": 1416.0, "attn_l0_us": 226.0}


def box_calibration(dev, seconds=1.0):
    """the pool's boxes read 8.95-9.47 ms for ONE build (device-to-device clock / power spread), so a driver line
    from one box cannot resolve a 1 % change.  Two fixed probes, ~1 s each, BEFORE the timed region on the same device: the 8192^3 fp16 GEMM
    on csrc/gemm256.hip (MFMA-dense, power-limited: tracks the clock the part holds) and the UNet's L0 self-attention shape (2 x 8 heads x 8192^2
    tokens, D = 40) on csrc/attention.hip (the step's largest single launch).  `speed_index` = mean of (gemm TFLOP/s / reference) and
    (reference attention us / attention us); `denoise_step_ms_normalised` = the measured step x speed_index - what the reference box would
    read.  The raw figure stays the headline."""
    import ctypes as C
    from blobctrl_amd import _lib
    from blobctrl_amd.launch import Recorder
    lib = _lib.load()
    rec = Recorder(dev)
    gen = torch.Generator(device="cpu").manual_seed(7)
    n = 8192
    A = (torch.randn(n, n, generator=gen) * 0.5).half().to(dev)
    W = (torch.randn(n, n, generator=gen) * 0.02).half().to(dev)
    seg_g = rec.begin("cal_gemm")
    rec.gemm(A=A, W=W, M=n, N=n, K=n, out=rec.empty(n, n), tile_cfg=_lib.TILE_G256)
    B, heads, d, N = 2, 8, 40, 8192
    qk = (torch.randn(B * N, 2 * heads * d, generator=gen)).half().to(dev)
    vt = (torch.randn(B, heads * d, N, generator=gen)).half().to(dev)
    seg_a = rec.begin("cal_attn")
    C_ = heads * d
    rec.attention(qk, qk, vt, rec.empty(B * N, C_), B, heads, d, N, N, 2 * C_, 2 * C_, N, C_, N * 2 * C_, N * 2 * C_, C_ * N, N * C_, d ** -0.5, q_off=0, k_off=C_)
    # (third probe, round 6 late: the two above read within 1 % on boxes whose batch-1 steps were 2.3 % apart - that step is made of launches
    #  that do NOT fill the chip) a chain of 32 dependent [1024 x 1280 x 1280] projections: launch gap + the latency of a small grid
    xc = (torch.randn(1024, 1280, generator=gen) * 0.5).half().to(dev)
    Wc = (torch.randn(1280, 1280, generator=gen) * 0.03).half().to(dev)
    seg_c = rec.begin("cal_chain")
    cur = xc
    for _ in range(32):
        nxt = rec.empty(1024, 1280)
        rec.gemm(A=cur, W=Wc, M=1024, N=1280, K=1280, out=nxt)
        cur = nxt
    s = torch.cuda.current_stream(dev).cuda_stream

    def time_seg(seg, budget):
        for _ in range(3):
            seg.run(s)
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps, spent, best = 0, 0.0, []
        while spent < budget:
            e0.record()
            for _ in range(10):
                seg.run(s)
            e1.record()
            torch.cuda.synchronize(dev)
            ms = e0.elapsed_time(e1) / 10
            best.append(ms)
            spent += ms * 10e-3
            reps += 10
        best.sort()
        return best[len(best) // 2], reps
    g_ms, g_reps = time_seg(seg_g, seconds)
    a_ms, a_reps = time_seg(seg_a, seconds)
    c_ms, c_reps = time_seg(seg_c, 0.5 * seconds)
    rec.close()
    out = {"gemm_8192_tflops": round(2.0 * n ** 3 / (g_ms * 1e-3) / 1e12, 1), "attn_l0_us": round(a_ms * 1e3, 1),
           "chain_us_per_launch": round(c_ms * 1e3 / 32, 2), "reference": CAL_REF, "launches": [g_reps, a_reps, c_reps]}
    out["speed_index"] = round(0.5 * (out["gemm_8192_tflops"] / CAL_REF["gemm_8192_tflops"] + CAL_REF["attn_l0_us"] / out["attn_l0_us"]), 4)
    if CAL_REF.get("chain_us_per_launch"):
        out["latency_index"] = round(CAL_REF["chain_us_per_launch"] / out["chain_us_per_launch"], 4)
    return out


def end_to_end(pw_u, pw_b, ucfg, bcfg, dev, res, denoise_steps, reps=3, batch=1):
    """One complete edit as scripts/blobctrl_inference.py runs it (UniPC, guidance window [0, 0.9], CFG 7.5), every stage on the
    clock: Gaussian-blob splat + DINOv2 ViT-L/14 on the 224^2 crop + CLIP text encoder (prompt and negative prompt) + 2 VAE encodes
    + the denoise loop (45 BlobNet-active + 5 UNet-only steps) + VAE decode.  Seeded synthetic weights of the real architectures;
    inputs are device tensors (image decoding / tokenisation stay on the host).  Median of `reps` edits after one warm-up edit."""
    import statistics
    import numpy as np
    from blobctrl_amd import synth
    from blobctrl_amd.clip_text import CLIPTextModel
    from blobctrl_amd.dinov2 import Dinov2Model
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from blobctrl_amd.splat import blob_dict_from_ellipse, splat_features
    from blobctrl_amd.vae import AutoencoderKL
    vae = AutoencoderKL(synth.synth_state_dict(synth.vae_param_shapes(), 33), device=str(dev))
    clip = CLIPTextModel(synth.synth_state_dict(synth.clip_text_param_shapes(), 88), num_heads=12, device=str(dev))
    dino = Dinov2Model(synth.synth_state_dict(synth.dinov2_param_shapes(1024, 24, 4, 14, 37 * 37), 99), num_heads=16, device=str(dev))
    eng = BlobCtrlEngine(pw_u, pw_b, ucfg, bcfg, device=str(dev), scheduler="unipc", vae=vae, text_encoder=clip)
    rng = np.random.Generator(np.random.PCG64(0))
    fg = torch.from_numpy(rng.uniform(-1, 1, (1, 3, res, res)).astype(np.float32)).to(dev)
    bg = torch.from_numpy(rng.uniform(-1, 1, (1, 3, res, res)).astype(np.float32)).to(dev)
    crop = torch.from_numpy(rng.standard_normal((1, 3, 224, 224)).astype(np.float32)).to(dev)      # processor output (host side)
    ids = torch.from_numpy(rng.integers(0, 49408, size=(2, 1, 77)).astype(np.int64)).repeat(1, batch, 1).to(dev)   # prompt=[scene_prompt] * num_samples (inf:196)
    sc = res / 512.0
    blob = blob_dict_from_ellipse([[361.1067 * sc, 367.8526 * sc], [85.4812 * sc, 103.6543 * sc], 87.3739], res, res)

    def sync():
        torch.cuda.synchronize()
        return time.perf_counter()

    def one():
        t = [sync()]
        score = splat_features(**blob, score_size=(res // 8, res // 8), return_d_score=True, device=str(dev))
        t.append(sync())
        feats = dino(crop).pooler_output.view(1, 1, -1)
        t.append(sync())
        prompt = eng.encode_prompt(ids[1], ids[0])
        t.append(sync())
        fl, bl = eng.encode_latents(fg, torch.Generator().manual_seed(1)), eng.encode_latents(bg, torch.Generator().manual_seed(2))
        t.append(sync())
        lat = eng(prompt, fl, bl, score, feats, num_inference_steps=denoise_steps, guidance_scale=7.5,
                  generator=torch.Generator().manual_seed(0), blobnet_conditioning_scale=1.0, blobnet_control_guidance_end=0.9)
        t.append(sync())
        img = eng.decode_latents(lat, "pt")
        t.append(sync())
        assert torch.isfinite(img).all()
        return [1e3 * (b - a) for a, b in zip(t[:-1], t[1:])]

    one()
    runs = [one() for _ in range(reps)]
    med = [statistics.median(r[k] for r in runs) for k in range(6)]
    names = ["splat_ms", "dinov2_ms", "clip_text_ms", "vae_encode_x2_ms", "denoise_loop_ms", "vae_decode_ms"]
    out = {n: round(v, 3) for n, v in zip(names, med)}
    out["edit_ms_end_to_end"] = round(statistics.median(sum(r) for r in runs), 2)
    out["config"] = f"{res}x{res}, {denoise_steps} UniPC steps, guidance window [0, 0.9] (script defaults, inf:300-307), CFG 7.5, batch {batch}"
    if batch > 1:
        P = eng.plan_for(batch, res // 8, res // 8, 77, 768, denoise_steps)
        from blobctrl_amd.pipeline import blobnet_keep
        active = sum(1 for k in blobnet_keep(denoise_steps, 0.0, 0.9) if k != 0.0)
        flops = P.step_active.flops * active + P.step_inactive.flops * (denoise_steps - active)
        out["denoise_step_ms"] = round(out["denoise_loop_ms"] / denoise_steps, 3)
        out["images_per_s"] = round(batch / (out["edit_ms_end_to_end"] * 1e-3), 4)
        out["loop_frac_of_peak"] = round(flops / (out["denoise_loop_ms"] * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4)
    return out


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def visible_gpu_count():
    """GPUs this process tree may use, WITHOUT touching HIP or torch (the launcher parent must stay GPU-free by construction: a
    fork + exec of a GPU-initialised process takes the box down on this pool).  HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES /
    CUDA_VISIBLE_DEVICES when set, else the KFD topology in sysfs (nodes with simd_count > 0 are GPUs)."""
    for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            return len([x for x in v.split(",") if x.strip() != ""])
    n = 0
    root = "/sys/class/kfd/kfd/topology/nodes"
    try:
        for node in os.listdir(root):
            try:
                with open(os.path.join(root, node, "properties")) as f:
                    props = dict(ln.split()[:2] for ln in f if len(ln.split()) >= 2)
                n += int(props.get("simd_count", "0")) > 0
            except OSError:
                pass
    except OSError:
        return 0
    return n


def launch_ranks(n, argv):
    """`python bench.py --gpus N` without torchrun: start N fresh worker processes (one per GPU, LOCAL_RANK = GPU index) from
    this parent, which has made NO GPU call (never re-exec a process that touched the GPU), relay rank 0's JSON line, and
    fail if any worker fails.  With fewer than N GPUs visible (a 1-GPU box) the workers share devices and use gloo, because
    RCCL refuses two ranks on one device; BC_DIST_BACKEND overrides."""
    import subprocess
    ngpu = visible_gpu_count()                  # sysfs / environment only: the parent makes no HIP and no torch GPU call
    env = dict(os.environ, WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    if "BC_DIST_BACKEND" not in env and ngpu < n:
        env["BC_DIST_BACKEND"] = "gloo"
    procs = []
    for r in range(n):
        e = dict(env, RANK=str(r), LOCAL_RANK=str(r))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=e,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=True))
    out0, _ = procs[0].communicate()
    codes = [procs[0].returncode] + [p.wait() for p in procs[1:]]
    lines = [ln for ln in (out0 or "").splitlines() if ln.startswith("{")]
    if any(codes) or not lines:
        sys.stderr.write(f"bench.py: worker exit codes {codes}\n")
        sys.stdout.write(out0 or "")
        sys.exit(1)
    print(lines[-1], flush=True)
    sys.exit(0)


def stub_worker(args):
    """BC_BENCH_STUB=1: the launcher / rendezvous / max-over-ranks plumbing without a GPU (CPU test of `--gpus N`)."""
    from blobctrl_amd import dist as bdist
    import torch.distributed as tdist
    rank, world, local = bdist.init_from_env("gloo")
    mine = bdist.shard_requests(args.requests, rank, world) if args.requests else list(range(args.steps))
    dt = bdist.barrier_max_seconds(0.01 * (1 + rank))
    total = args.requests if args.requests else world * args.steps
    ident = dict(rank=rank, local_rank=local, backend=(tdist.get_backend() if world > 1 else None), local_device=local, pci_bdf=None)
    ranks = [ident]
    if world > 1:
        ranks = [None] * world
        tdist.all_gather_object(ranks, ident)
    if rank == 0:
        print(json.dumps({"metric": "stub", "value": total / dt, "n_gpus": world, "steps": args.steps, "local_requests": len(mine),
                          "gpus_arg": args.gpus, "metric_name": metric_name(args),
                          "config": {"ranks": ranks, "distinct_devices": len({r["local_device"] for r in ranks}),
                                     "workload": f"BASELINE configs[{3 if args.requests else 1}]"}}), flush=True)
    if world > 1:
        tdist.barrier()
        tdist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3, help="timed edits per rank (one edit = 50 denoise steps)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--denoise-steps", type=int, default=50)
    ap.add_argument("--scheduler", default="ddim", choices=["ddim", "unipc"])
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--batch", type=int, default=1, help="images per edit (BASELINE configs[2]/[4] use 8 / 4; headline = 1)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-e2e", action="store_true", help="skip the end-to-end (splat + DINOv2 + CLIP + VAE + loop) timing")
    ap.add_argument("--no-configs", action="store_true", help="skip the C3 / C5 / other-scheduler timings (`configs` block of the line)")
    ap.add_argument("--table", action="store_true", help="print the per-kernel event-time table to stderr")
    ap.add_argument("--no-calibration", action="store_true", help="skip the ~2 s box calibration probes in front of the timed region")
    ap.add_argument("--requests", type=int, default=0,
                    help="BASELINE configs[3]: this many independent edit requests in total, sharded round-robin over the ranks "
                         "(dist.shard_requests) and run `--batch` at a time as per-request batches; 0 = `--steps` edits per rank")
    ap.add_argument("--full", action="store_true",
                    help="also run the optional blocks (CPU baseline, box calibration, roofline, other configurations, end to end); each "
                         "can still be left out by its --no-* option.  Without --full only the headline is measured")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the final latents of the last timed edit (rank 0) as DIR/latents.npy (float32)")
    ap.add_argument("--cpu-baseline-worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full:                                  # a plain run: the headline only
        args.no_cpu_baseline = args.no_calibration = args.no_roofline = args.no_configs = args.no_e2e = True

    if args.cpu_baseline_worker:                       # child of a bench run: CPU only (see start_cpu_baseline)
        return cpu_baseline_worker(args.res // 8, args.res // 8, args.denoise_steps)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        launch_ranks(args.gpus, sys.argv[1:])          # never returns
    if os.environ.get("BC_BENCH_STUB"):
        return stub_worker(args)

    from blobctrl_amd import dist as bdist
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from blobctrl_amd.splat import splat_features
    from blobctrl_amd.weights import PackedTrunk
    import torch.distributed as tdist

    cpu_handle = None
    if "WORLD_SIZE" not in os.environ and args.gpus == 1 and not args.no_cpu_baseline and args.batch == 1 and not os.environ.get("BC_BENCH_STUB"):
        cpu_handle = start_cpu_baseline(args.res // 8, args.res // 8, args.denoise_steps)      # (before the first GPU call of this process)
    rank, world, local = bdist.init_from_env(os.environ.get("BC_DIST_BACKEND"))
    if args.gpus != world:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch with torchrun --nproc-per-node {args.gpus} "
                         f"or let `python bench.py --gpus {args.gpus}` start the ranks itself (WORLD_SIZE unset)")
    dev = torch.device(f"cuda:{local % max(1, torch.cuda.device_count())}")   # (modulo: lets a 1-GPU box exercise N > 1 with gloo)
    torch.cuda.set_device(dev)
    ucfg, bcfg = full_configs()
    h = w = args.res // 8
    state = {}

    def build_unet():
        state["usd"], state["bsd"] = synth_weights()
        return PackedTrunk(state["usd"], dev, ucfg.block_out_channels)

    def build_blob():
        return PackedTrunk(state["bsd"], dev, bcfg.block_out_channels)

    t0 = time.perf_counter()
    pw_u = bdist.broadcast_packed(build_unet, dev)          # rank 0 packs, RCCL broadcast over xGMI to the others
    pw_b = bdist.broadcast_packed(build_blob, dev)
    t_weights = time.perf_counter() - t0
    cal = None
    if rank == 0 and not args.no_calibration:
        try:
            cal = box_calibration(dev)
        except Exception as e:                                                  # noqa: BLE001  (optional detail: must not lose the line)
            cal = {"error": f"{type(e).__name__}: {e}"[:300]}
    pipe = BlobCtrlEngine(pw_u, pw_b, ucfg, bcfg, device=str(dev), scheduler=args.scheduler)
    inp = synth_inputs(h, w, batch=args.batch)
    inp_dev = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}     # inputs resident in HBM
    score = splat_features(**inp["blob"], score_size=(h, w), return_d_score=True, device=str(dev))   # HIP rasteriser

    def one_edit(seed_off=0):
        lat = inp_dev["latents"] if seed_off == 0 else torch.roll(inp_dev["latents"], seed_off, -1)
        return pipe(inp_dev["prompt"], inp_dev["fg"], inp_dev["bg"], score, inp_dev["dino"], num_inference_steps=args.denoise_steps,
                    guidance_scale=7.5, latents=lat, blobnet_conditioning_scale=1.0,
                    blobnet_control_guidance_start=0.0, blobnet_control_guidance_end=1.0)

    request_batch = lambda ids: make_request_batch(ids, h, w, dev)

    def run_requests(rb):
        return pipe(rb["prompt"], rb["fg"], rb["bg"], rb["score"], rb["dino"], num_inference_steps=args.denoise_steps,
                    guidance_scale=7.5, latents=rb["latents"], blobnet_conditioning_scale=rb["strength"],
                    blobnet_control_guidance_start=0.0, blobnet_control_guidance_end=1.0)

    if args.requests:
        mine = bdist.shard_requests(args.requests, rank, world)              # round-robin, no data-path collective
        batches = [request_batch(mine[i:i + args.batch]) for i in range(0, len(mine), args.batch)]   # resident in HBM
        for _ in range(max(1, args.warmup)):
            out = run_requests(batches[0])
    else:
        for i in range(max(1, args.warmup)):
            out = one_edit(i)
    assert torch.isfinite(out).all(), "non-finite latents"
    if world > 1:
        tdist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if args.requests:
        for rb in batches:
            out = run_requests(rb)
    else:
        for i in range(args.steps):
            out = one_edit(rank * 1000 + i + 1)
    torch.cuda.synchronize()
    if world > 1:
        tdist.barrier()
    dt = bdist.barrier_max_seconds(time.perf_counter() - t0, dev)
    if args.dump_outputs and rank == 0:
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "latents.npy"), out.detach().float().cpu().numpy())
    # The CPU baseline runs beside the optional blocks below (never beside the timed region above).  Its worker is pinned to socket 0:
    # move this process (host side of the roofline / configs / end-to-end blocks) OFF those CPUs first, and say in the line what ran
    # beside what.
    cpu_overlap = None
    if cpu_handle is not None:
        try:
            mine = set(os.sched_getaffinity(0))
            other = sorted(mine - set(socket0_cpus()))
            if other:
                os.sched_setaffinity(0, other)
                cpu_overlap = (f"the bench process moved to the {len(other)} CPUs outside socket 0 before the worker was released; the worker's steps "
                               "ran beside the roofline / configs / end-to-end blocks of this line (GPU-bound; host side on the other socket)")
            else:
                cpu_overlap = ("single-socket host: the worker's steps ran beside the host side of the roofline / configs / end-to-end blocks on "
                               "the SAME CPUs (those blocks are GPU-bound; their host threads are few)")
        except (AttributeError, OSError) as e:
            cpu_overlap = f"affinity not available ({e}): the worker's steps ran beside the optional blocks, unpinned parent"
    release_cpu_baseline(cpu_handle)
    weights_s = [round(t_weights, 2)]
    ident = dict(rank=rank, local_rank=local, backend=(tdist.get_backend() if world > 1 else None), **device_identity(dev))
    ranks = [ident]
    if world > 1:
        weights_s = [None] * world
        tdist.all_gather_object(weights_s, round(t_weights, 2))
        ranks = [None] * world
        tdist.all_gather_object(ranks, ident)
    units = args.requests if args.requests else world * args.steps * args.batch
    # every rank's copy of the broadcast weight arenas hashed on the device: rank r > 0 holds what rank 0 packed
    wsha = None
    if world > 1:
        wsha = [None] * world
        tdist.all_gather_object(wsha, bdist.arena_hash(pw_u, pw_b))

    plan = pipe.plan_for(args.batch, h, w, 77, 768, args.denoise_steps, per_request=bool(args.requests))
    line = {
        "metric": metric_name(args),
        "value": units / dt, "unit": "edits/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / (len(batches) if args.requests else args.steps) * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "fp16", "data": "synthetic",
        "config": {"workload": f"BASELINE configs[{(3 if args.requests else 1 if args.batch == 1 else 2) if args.res == 512 else 4}]: "
                               f"{args.res}x{args.res} edit, batch {args.batch} (CFG batch {2 * args.batch} for the UNet, "
                               f"BlobNet shared across CFG halves), {args.denoise_steps} {args.scheduler.upper()} steps, "
                               "guidance window [0,1], fp16 activations / fp32 accumulate, LoRA pre-merged, hipGraph-replayed steps",
                   "edits_per_rank": (len(mine) if args.requests else args.steps * args.batch), "denoise_steps": args.denoise_steps,
                   "requests_total": args.requests or None, "per_request_batches": bool(args.requests),
                   "denoise_step_ms": dt / (len(batches) if args.requests else args.steps) / args.denoise_steps * 1e3,
                   "algorithmic_tflop_per_edit": plan.step_active.flops * args.denoise_steps / 1e12 / args.batch,
                   "dist_backend": (tdist.get_backend() if world > 1 else None),
                   "rccl_version": (".".join(str(x) for x in torch.cuda.nccl.version()) if world > 1 and tdist.get_backend() == "nccl" else None),
                   "nranks_seen": len(ranks), "weights_sha16": wsha,
                   "ranks": ranks, "distinct_devices": len({(r["local_device"], r["pci_bdf"]) for r in ranks}),
                   "weights_s": weights_s,
                   # which plan this line measured: planner options that differ from their defaults (BC_PLAN,
                   # blobctrl_amd/options.py) and the launches per kernel instantiation of ONE BlobNet-active step
                   # plan / whole-edit-graph cache traffic of this rank's engine over warm-up + timed region: a --requests run must show ONE
                   # recorded plan and ONE captured graph however many per-request batches it replayed
                   "plan_cache": dict(pipe.cache_stats),
                   "plan": {"options_non_default": plan.options_non_default, "launches_per_active_step": len(plan.step_active.meta),
                            "variants": plan_variants(plan)}},
    }
    if cal is not None:
        line["box_calibration"] = cal
        if "speed_index" in cal:
            line["config"]["denoise_step_ms_normalised"] = round(line["config"]["denoise_step_ms"] * cal["speed_index"], 4)
    # The headline numbers above are complete.  Everything below is optional detail: a failure there is recorded in the line, it must
    # not lose the line.
    def guarded(key, fn):
        try:
            return fn()
        except Exception as e:                                              # noqa: BLE001
            line.setdefault("errors", {})[key] = f"{type(e).__name__}: {e}"[:300]
            return None
    if rank == 0 and not args.no_roofline:
        r = guarded("roofline", lambda: roofline(pipe, plan, args.res, args.batch))
        if r is not None:
            line["roofline"] = r[0]
            if args.table:
                print(json.dumps(r[1], indent=1), file=sys.stderr)
    if rank == 0 and world == 1 and not args.no_configs and args.batch == 1 and not args.requests and args.res == 512:
        c = guarded("configs", lambda: other_configs(pipe, pw_u, pw_b, ucfg, bcfg, dev, args.denoise_steps, args.scheduler))
        if c is not None:
            line["configs"] = c
    if rank == 0 and world == 1 and not args.no_e2e and args.batch == 1 and not args.requests:
        e2e = guarded("end_to_end", lambda: end_to_end(pw_u, pw_b, ucfg, bcfg, dev, args.res, args.denoise_steps))
        if e2e is not None:
            line["edit_ms_end_to_end"] = e2e["edit_ms_end_to_end"]
            line["end_to_end"] = e2e
    if rank == 0 and world == 1 and not args.no_e2e and not args.no_configs and args.batch == 1 and not args.requests and args.res == 512:
        # what `python scripts/blobctrl_inference.py` runs with no arguments (inf:276,304-311): num_samples = 2 (prompt = [scene_prompt] * 2:
        # two variations of ONE edit in a batch), UniPC, guidance window [0, 0.9], 50 steps - end to end
        sd = guarded("script_default", lambda: end_to_end(pw_u, pw_b, ucfg, bcfg, dev, args.res, args.denoise_steps, reps=3, batch=2))
        if sd is not None:
            line.setdefault("configs", {})["script_default"] = sd
    if cpu_handle is not None:
        line["cpu_baseline"] = collect_cpu_baseline(cpu_handle)
        line["cpu_baseline"]["beside"] = cpu_overlap
    if rank == 0:
        print(json.dumps(line), flush=True)
    if world > 1:
        tdist.barrier()
        tdist.destroy_process_group()


if __name__ == "__main__":
    main()
