"""DPM-Solver++ on MI355X: the third-order step kernel (bc_cfg_scheduler_step3) and the two existing step kernels driven by DPM-Solver
tables, the tiny-net loop against the REFERENCE's own DPM-Solver loops (tests/golden/loop_tiny_dpm.npz), the reference pipeline's own
`__call__(timesteps=[...], generator=)` with an SDE-DPM-Solver++ scheduler (pipeline_call_dpm.npz), and the plan / graph cache when the
scheduler changes between UniPC and DPM-Solver++ 2M.

Bars (fixed before measuring, those of tests/test_kernels_gpu.py:516-544 and tests/test_ddim_eta_gpu.py:126-222): kernel max-abs <= 1e-6
of max |ref| against an fp64 host evaluation; tiny loop (teacher-forced guided eps and free-running final latents) max-abs / scale
< 1e-2 and PSNR > 40 dB; end-to-end __call__ < 3e-2 and > 36 dB."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.common import PIPE, TINY, FakeTokenizer, g, pipeline_cases, psnr, tiny_pipeline_weights, tiny_weights  # noqa: E402
from tests.gpu_common import launch_step, make_pipeline, tiny_trunk_configs  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000, steps_offset=1)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


# ------------------------------------------------------------------------------------------------------------------ kernels
def _host_step(c, eps_tok, x, hist, noise, guidance, B, h, w):
    """fp64 crop + CFG + one table row (+ c12 * noise, + c13 * x0_{i-2})."""
    c = c.double()
    e4 = eps_tok.double().reshape(2 * B, h, 2 * w, 4)[:, :, w:, :].permute(0, 3, 1, 2)
    eu, ec = e4[:B], e4[B:]
    gs = guidance if guidance >= 0 else float(c[11])
    e = eu + gs * (ec - eu)
    n = B * 4 * h * w
    m0, m1, last = (hist.double()[k].reshape(B, 4, h, w) for k in range(3))
    xd = x.double()
    x0 = xd * c[0] - e * c[1]
    xc = c[3] * last + c[4] * m0 + c[5] * m1 + c[6] * x0 if c[2] != 0 else xd
    xn = c[7] * xc + c[8] * x0 + c[9] * m0 + c[10] * e + c[13] * m1
    if noise is not None:
        xn = xn + c[12] * noise.double()
    return xn, torch.stack([x0.reshape(n), m0.reshape(n), xc.reshape(n)]), e


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("form", ["step", "noise", "step3"])
def test_step_kernels_on_dpm_tables(B, form):
    """Each step kernel against the schedulers_dpm.npz trajectories (CFG 7.5 with a garbage left half) and its host row."""
    from blobctrl_amd import _lib
    from blobctrl_amd.schedulers import DPMSolverMultistepTable
    lib = _lib.load()
    dev = "cuda:0"
    z = np.load(os.path.join(GOLD, "schedulers_dpm.npz"))
    name = {"step": "pp2_mid_karras_50", "noise": "sde2_mid_lin_15", "step3": "pp3_lin_14"}[form]
    kw = json.loads(str(z[f"{name}_kw"]))
    n_ = kw.pop("n")
    kw.pop("timesteps")
    tab = DPMSolverMultistepTable(**{k: v for k, v in dict(SD, **kw).items() if k != "beta_schedule"}).set_timesteps(n_)
    ref = z[f"{name}_traj"]
    nsteps = ref.shape[0] - 1
    h = w = 8
    n = B * 4 * h * w
    coef = tab.coef.clone()
    coef[:, 11] = 7.5
    coef = coef.to(dev)
    noise = torch.stack([g(200 + i, 1, 4, h, w).repeat(B, 1, 1, 1) for i in range(nsteps)]).to(dev)
    x = torch.from_numpy(ref[0]).repeat(B, 1, 1, 1).to(dev).contiguous()
    hist = torch.zeros(3, n, device=dev)
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    eps_out = torch.zeros(B, 4, h, w, device=dev)

    def launch(eps, guidance=-1.0, advance=1):
        _lib.check(launch_step(lib, form, eps, x, coef, idx, hist, guidance, B, h, w, eps_out, advance, noise=noise, nsteps=nsteps), form)
        torch.cuda.synchronize()

    worst = 0.0
    for i in range(nsteps):
        # eps token-major [2B][h][2w][4]: the right half holds uncond u and cond c with u + 7.5 (c - u) = the fixture's eps_i
        e = g(100 + i, 1, 4, h, w)[0].permute(1, 2, 0)
        u = g(300 + i, 1, h, w, 4)[0]
        tok = torch.randn(2 * B, h, 2 * w, 4, generator=torch.Generator().manual_seed(400 + i)) * 50     # garbage left half
        tok[:B, :, w:] = u
        tok[B:, :, w:] = u + (e - u) / 7.5
        tok = tok.to(dev)
        x_in, hist_in = x.clone().cpu(), hist.clone().cpu()
        launch(tok)
        xn, hist_ref, eh = _host_step(coef[i].cpu(), tok.cpu(), x_in, hist_in, noise[i].cpu() if form == "noise" else None, -1.0, B, h, w)
        for got, r_, what in ((x, xn, "latents"), (hist, hist_ref, "hist"), (eps_out, eh, "eps_out")):
            err = (got.cpu().double() - r_.reshape(got.shape)).abs().max().item()
            assert err <= 1e-6 * r_.abs().max().item(), (form, B, i, what, err)
        for b in range(B):                          # test_kernels_gpu.py:544: rtol 2e-5, atol 2e-5 * max |ref|
            got, r_ = x[b:b + 1].cpu().numpy().astype(np.float64), ref[i + 1].astype(np.float64)
            worst = max(worst, rel_err(got, r_))
            assert (np.abs(got - r_) <= 2e-5 * np.abs(r_) + 2e-5 * np.abs(r_).max()).all(), (form, B, i, b, rel_err(got, r_))
    print(f"{form} B={B} ({name}): worst per-step rel err vs the reference trajectory {worst:.2e}")
    # a step index at or past the table (capture warm-ups) leaves every buffer untouched (the plain step has no nsteps argument)
    if form != "step":
        for step in (nsteps, nsteps + 2):
            idx.fill_(step)
            x0_, h0_, e0_ = x.clone(), hist.clone(), eps_out.clone()
            launch(tok)
            assert torch.equal(x, x0_) and torch.equal(hist, h0_) and torch.equal(eps_out, e0_) and int(idx.item()) == step + 1


# ------------------------------------------------------------------------------------------------------------------ tiny loop
def _loop_inputs():
    from oracle import blob_splat
    score = torch.from_numpy(blob_splat.splat_scores_from_ellipse([[40.0, 42.0], [20.0, 30.0], 25.0], 64, 64, 8, 8))
    return dict(latents=g(31, 1, 4, 8, 8), prompt=g(32, 2, 7, TINY["ctx"]), fg=g(33, 1, 4, 8, 8) * 0.18215 * 5,
                bg=g(34, 1, 4, 8, 8) * 0.18215 * 5, score=score, dino=g(35, 1, 1, TINY["feat"]))


def _use(eng, **kw):
    from blobctrl_amd.schedulers import DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler(**dict(SD, **kw))
    eng.set_scheduler(s.kind, s.table_params())
    return s


@pytest.mark.parametrize("tag", ["karras2m_6", "sde2m_5", "dpm3m_6", "custom2m_10"])
@pytest.mark.parametrize("graphs", [False, True])
def test_dpm_loop_matches_the_reference(tag, graphs):
    z = np.load(os.path.join(GOLD, "loop_tiny_dpm.npz"))
    usd, bsd = tiny_weights()
    kw = json.loads(str(z[f"{tag}_kw"]))
    steps, ts = kw.pop("n"), kw.pop("timesteps")
    gs, ge = [float(v) for v in z[f"{tag}_window"]]
    sde = f"{tag}_noise" in z.files
    a = _loop_inputs()
    eng = make_pipeline(usd, bsd, scheduler="unipc", use_graphs=graphs)
    _use(eng, **kw)
    extra = dict(timesteps=ts) if ts is not None else {}
    gen = (lambda: torch.Generator().manual_seed(int(z[f"{tag}_seed"]))) if sde else (lambda: None)
    run = lambda **k: eng.denoise(a["prompt"], a["fg"], a["bg"], a["score"], a["dino"], num_inference_steps=steps, guidance_scale=7.5,
                                  latents=a["latents"], blobnet_control_guidance_start=gs, blobnet_control_guidance_end=ge, **extra, **k)
    # (i) teacher-forced: the reference's latents entering every step, its guided eps out
    trace = []
    run(trace=trace, teacher_latents=[torch.from_numpy(v) for v in z[f"{tag}_lat"]], generator=gen())
    assert np.array_equal(eng.timesteps.numpy(), z[f"{tag}_timesteps"])
    for i, (eps_gpu, _) in enumerate(trace):
        ref = z[f"{tag}_eps"][i]
        e = rel_err(eps_gpu.cpu().numpy(), ref)
        assert e < 1e-2 and psnr(eps_gpu.cpu().numpy(), ref) > 40.0, f"step {i}: guided eps rel err {e:.3e}"
    # (ii) free-running against the reference's final latents
    out = run(generator=gen()).cpu().numpy()
    ref = z[f"{tag}_final"]
    print(f"{tag} graphs {graphs}: free-running final latents rel err {rel_err(out, ref):.3e}, PSNR {psnr(out, ref):.1f} dB")
    assert rel_err(out, ref) < 1e-2 and psnr(out, ref) > 40.0
    if sde:                                         # the tapped noise as variance_noise: bit-identical to the generator run
        out2 = run(variance_noise=torch.from_numpy(z[f"{tag}_noise"])).cpu().numpy()
        assert np.array_equal(out, out2)
        with pytest.raises(NotImplementedError, match="DDIM"):
            run(eta=0.5)


def test_request_batch_with_one_generator_per_request():
    usd, bsd = tiny_weights()
    eng = make_pipeline(usd, bsd, scheduler="unipc", use_graphs=True)
    _use(eng, algorithm_type="sde-dpmsolver++")
    a = _loop_inputs()
    B, steps = 3, 5
    prompts = [g(60 + k, 2, 7, TINY["ctx"]) for k in range(B)]
    lat = [g(70 + k, 1, 4, 8, 8) for k in range(B)]
    fg = [a["fg"] * (1.0 + 0.1 * k) for k in range(B)]
    seeds = [101, 202, 303]
    singles = [eng.denoise(prompts[k], fg[k], a["bg"], a["score"], a["dino"], num_inference_steps=steps, latents=lat[k],
                           generator=torch.Generator().manual_seed(seeds[k])).cpu().numpy() for k in range(B)]
    batch = eng.denoise(torch.cat([p[:1] for p in prompts] + [p[1:] for p in prompts]), torch.cat(fg), a["bg"].repeat(B, 1, 1, 1),
                        a["score"].repeat(B, 1, 1, 1), a["dino"].repeat(B, 1, 1), num_inference_steps=steps, latents=torch.cat(lat),
                        blobnet_conditioning_scale=[1.0] * B, generator=[torch.Generator().manual_seed(s) for s in seeds]).cpu().numpy()
    for k in range(B):
        r = rel_err(batch[k:k + 1], singles[k])
        print(f"request {k}: batch vs single edit max-abs/scale {r:.3e}")
        assert r < 1e-2 and psnr(batch[k:k + 1], singles[k]) > 40.0
    assert rel_err(singles[0], singles[1]) > 1e-2                                     # per-sample noise really differs


# ------------------------------------------------------------------------------------------------------------------ __call__
@pytest.fixture(scope="module")
def parts():
    from blobctrl_amd.clip_text import CLIPTextModel
    from blobctrl_amd.dinov2 import Dinov2Model
    from blobctrl_amd.modules import BlobNetModel, UNet2DConditionModel
    from blobctrl_amd.vae import AutoencoderKL
    usd, bsd = tiny_weights()
    ucfg, bcfg = tiny_trunk_configs()
    vsd, csd, dsd = tiny_pipeline_weights()
    return dict(unet=UNet2DConditionModel(usd, ucfg), blobnet=BlobNetModel(bsd, bcfg),
                vae=AutoencoderKL(vsd, norm_num_groups=PIPE["vae_groups"]),
                text_encoder=CLIPTextModel(csd, num_heads=PIPE["clip"]["heads"]),
                dinov2=Dinov2Model(dsd, num_heads=PIPE["dino"]["heads"], patch_size=PIPE["dino"]["patch"]))


def test_pipeline_call_with_dpm_timesteps_matches_the_reference_call(parts):
    from PIL import Image
    from blobctrl_amd.pipeline import StableDiffusionBlobNetPipeline
    from blobctrl_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler
    z = np.load(os.path.join(GOLD, "pipeline_call.npz"))
    zd = np.load(os.path.join(GOLD, "pipeline_call_dpm.npz"))
    kw = dict(pipeline_cases()["ddim_neg2"])
    for k in ("scheduler", "seed", "rng_seed", "num_inference_steps"):
        kw.pop(k)
    seed, rng_seed, ts = int(zd["seed"]), int(zd["rng_seed"]), [int(t) for t in zd["timesteps"]]
    sch = DPMSolverMultistepScheduler.from_config(DDIMScheduler(**SD).config, algorithm_type="sde-dpmsolver++")
    pipe = StableDiffusionBlobNetPipeline(tokenizer=FakeTokenizer(), scheduler=sch, safety_checker=None, requires_safety_checker=False,
                                          **parts)
    common = dict(fg_image=Image.fromarray(z["fg"]), bg_image=Image.fromarray(z["bg"]), gs_score=torch.from_numpy(z["gs_score"]),
                  height=64, width=64, **kw)
    torch.manual_seed(rng_seed)
    out = pipe(timesteps=ts, generator=torch.Generator().manual_seed(seed), output_type="latent", **common)
    got, ref = out.images.cpu().numpy(), zd["latents"]
    assert pipe.num_timesteps == len(ts) and pipe.scheduler.timesteps.tolist() == zd["scheduler_timesteps"].tolist()
    rel = rel_err(got, ref)
    print(f"__call__ sde-dpm++ on {ts}: end to end max-abs/scale {rel:.3e}, PSNR {psnr(got, ref):.1f} dB")
    assert got.shape == ref.shape and rel < 3e-2 and psnr(got, ref) > 36.0
    # UniPC / DDIM keep refusing caller timesteps, as before
    pipe.scheduler = UniPCMultistepScheduler()
    with pytest.raises(NotImplementedError, match="timesteps"):
        pipe(timesteps=ts, generator=torch.Generator().manual_seed(seed), output_type="latent", **common)


# ------------------------------------------------------------------------------------------------------------------ caches
def test_unipc_dpm_unipc_reuses_the_plan_and_each_matches_its_reference():
    usd, bsd = tiny_weights()
    a = _loop_inputs()
    zl = np.load(os.path.join(GOLD, "loop_tiny.npz"))
    zd = np.load(os.path.join(GOLD, "loop_tiny_dpm.npz"))
    eng = make_pipeline(usd, bsd, scheduler="unipc", use_graphs=True)
    from blobctrl_amd.schedulers import UniPCMultistepScheduler
    u = UniPCMultistepScheduler()
    run = lambda ge: eng.denoise(a["prompt"], a["fg"], a["bg"], a["score"], a["dino"], num_inference_steps=6, guidance_scale=7.5,
                                 latents=a["latents"], blobnet_control_guidance_start=0.0, blobnet_control_guidance_end=ge).cpu().numpy()
    eng.set_scheduler(u.kind, u.table_params())
    x_u = run(0.67)
    st = dict(eng.cache_stats)
    _use(eng, use_karras_sigmas=True)
    x_d = run(0.67)
    eng.set_scheduler(u.kind, u.table_params())
    x_u2 = run(0.67)
    st2 = eng.cache_stats
    assert st2["plans_recorded"] == st["plans_recorded"] and st2["loop_graph_captures"] == st["loop_graph_captures"]
    assert st2["plan_hits"] == st["plan_hits"] + 2 and st2["loop_graph_hits"] == st["loop_graph_hits"] + 2
    for got, ref, what in ((x_u, zl["unipc_6_final"], "unipc"), (x_d, zd["karras2m_6_final"], "dpm++ 2m karras"),
                           (x_u2, zl["unipc_6_final"], "unipc again")):
        print(f"{what}: rel err {rel_err(got, ref):.3e}, PSNR {psnr(got, ref):.1f} dB")
        assert rel_err(got, ref) < 1e-2 and psnr(got, ref) > 40.0, what
    assert np.array_equal(x_u, x_u2)
