"""Stochastic DDIM (eta > 0) on MI355X: the noise step kernel (bc_cfg_scheduler_step_noise) against a host evaluation of its table
row, the tiny-net loop against the REFERENCE's own stochastic loop (tests/golden/loop_tiny_eta.npz) and the reference pipeline's own
`__call__(eta=1.0, generator=CPU generator)` (pipeline_call_eta.npz), the plan / whole-edit graph cache across seeds and etas, a
per-request batch with one generator per request, and the noise indexing of the full-size 512^2 plan of the benchmark.

Bars (fixed before measuring, those of tests/test_parity_gpu.py::test_denoise_loop_matches_reference and tests/test_pipeline_call_gpu.py):
tiny loop and loop-from-entry-tensors max-abs / scale < 1e-2 and PSNR > 40 dB; end-to-end __call__ < 3e-2 and > 36 dB; kernel
max-abs <= 1e-6 of max |ref|; full-size step arithmetic max-abs <= 1e-5 of max |x|."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.common import PIPE, TINY, FakeTokenizer, g, pipeline_cases, psnr, tiny_cfgs, tiny_pipeline_weights, tiny_weights  # noqa: E402
from tests.gpu_common import launch_step, make_pipeline, tiny_trunk_configs  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


# ------------------------------------------------------------------------------------------------------------------ kernel
def _host_step(coef_row, eps_tok, x, hist, noise, guidance, B, h, w):
    """fp64 evaluation of crop + CFG + one table row + c12 * noise (the kernel's arithmetic)."""
    c = coef_row.double()
    e4 = eps_tok.double().reshape(2 * B, h, 2 * w, 4)[:, :, w:, :].permute(0, 3, 1, 2)          # right half, NCHW
    eu, ec = e4[:B], e4[B:]
    gs = guidance if guidance >= 0 else float(c[11])
    e = eu + gs * (ec - eu)
    n = B * 4 * h * w
    m0, m1, last = (hist.double()[k].reshape(B, 4, h, w) for k in range(3))
    xd = x.double()
    x0 = xd * c[0] - e * c[1]
    xc = c[3] * last + c[4] * m0 + c[5] * m1 + c[6] * x0 if c[2] != 0 else xd
    xn = c[7] * xc + c[8] * x0 + c[9] * m0 + c[10] * e + c[12] * noise.double()
    return xn, torch.stack([x0.reshape(n), m0.reshape(n), xc.reshape(n)]), e


@pytest.mark.parametrize("B", [1, 3])
def test_noise_step_kernel_matches_its_table_row(B):
    from blobctrl_amd import _lib
    from blobctrl_amd.schedulers import DDIMTable, UniPCTable
    lib = _lib.load()
    dev = "cuda:0"
    h, w, nsteps = 5, 7, 6                                          # ragged canvas: n = B * 140 is no multiple of the block size
    n = B * 4 * h * w
    coef = DDIMTable().set_timesteps(nsteps, eta=1.0).coef.clone()
    coef[3] = UniPCTable().set_timesteps(nsteps).coef[3]             # one row with the corrector (history terms) on
    coef[3, 12] = 0.37
    coef[:, 11] = 7.5
    coef = coef.to(dev)
    eps = g(1, 2 * B, h, 2 * w, 4).to(dev)
    noise = g(2, nsteps, B, 4, h, w).to(dev)

    def run(step, guidance, advance=1):
        x = g(3 + step, B, 4, h, w).to(dev)
        hist = g(10 + step, 3, n).to(dev)
        eps_out = torch.full((B, 4, h, w), 123.0, device=dev)
        idx = torch.tensor([step], dtype=torch.int32, device=dev)
        x_in, hist_in = x.clone(), hist.clone()
        _lib.check(launch_step(lib, "noise", eps, x, coef, idx, hist, guidance, B, h, w, eps_out, advance, noise=noise, nsteps=nsteps),
                   "bc_cfg_scheduler_step_noise")
        torch.cuda.synchronize()
        assert int(idx.item()) == step + advance
        return x_in, hist_in, x, hist, eps_out

    for step, guidance in ((0, -1.0), (2, 1.0), (3, -1.0), (nsteps - 1, 5.0)):
        x_in, hist_in, x, hist, eps_out = run(step, guidance)
        xn, hist_ref, e = _host_step(coef[step].cpu(), eps.cpu(), x_in.cpu(), hist_in.cpu(), noise[step].cpu(), guidance, B, h, w)
        for got, ref, what in ((x, xn, "latents"), (hist, hist_ref, "hist"), (eps_out, e, "eps_out")):
            err = (got.cpu().double() - ref.reshape(got.shape)).abs().max().item()
            bar = 1e-6 * ref.abs().max().item()
            print(f"B={B} step {step} {what}: max-abs {err:.3e} (bar {bar:.3e})")
            assert err <= bar, (B, step, what, err, bar)
    # a step index at or past the table (the capture warm-ups advance the counter): nothing is read or written
    for step in (nsteps, nsteps + 3):
        x_in, hist_in, x, hist, eps_out = run(step, -1.0)
        assert torch.equal(x, x_in) and torch.equal(hist, hist_in) and (eps_out == 123.0).all()
    x_in, _, x, _, _ = run(1, -1.0, advance=0)
    assert not torch.equal(x, x_in)


# ------------------------------------------------------------------------------------------------------------------ tiny loop
def _loop_inputs():
    from oracle import blob_splat
    score = torch.from_numpy(blob_splat.splat_scores_from_ellipse([[40.0, 42.0], [20.0, 30.0], 25.0], 64, 64, 8, 8))
    return dict(latents=g(31, 1, 4, 8, 8), prompt=g(32, 2, 7, TINY["ctx"]), fg=g(33, 1, 4, 8, 8) * 0.18215 * 5,
                bg=g(34, 1, 4, 8, 8) * 0.18215 * 5, score=score, dino=g(35, 1, 1, TINY["feat"]))


class _StochasticDDIMOracle:
    """oracle.schedulers.DDIMOracle plus the eta > 0 terms of scheduling_ddim.py:253-261, 438-466 (given variance noise per step)."""

    def __init__(self, eta, noise):
        from oracle import schedulers as o_sched
        self.base, self.eta, self.noise = o_sched.DDIMOracle(), eta, noise
        self.init_noise_sigma = 1.0

    def set_timesteps(self, n):
        self.base.set_timesteps(n)
        self.timesteps = self.base.timesteps

    def step(self, model_output, sample):
        b = self.base
        i = b.step_index
        t = int(b.timesteps[i])
        prev_t = t - b.num_train // b.n
        a_t = b.alphas_cumprod[t]
        a_prev = b.alphas_cumprod[prev_t] if prev_t >= 0 else b.final_alpha_cumprod
        x0 = (sample - (1 - a_t) ** 0.5 * model_output) / a_t ** 0.5
        variance = ((1 - a_prev) / (1 - a_t)) * (1 - a_t / a_prev)
        std = self.eta * variance ** 0.5
        b.step_index += 1
        return a_prev ** 0.5 * x0 + (1 - a_prev - std ** 2) ** 0.5 * model_output + std * self.noise[i]


@pytest.mark.parametrize("tag", ["ddim_5", "ddim_6"])
@pytest.mark.parametrize("graphs", [False, True])
def test_stochastic_loop_matches_the_reference(tag, graphs):
    from oracle import pipeline as o_pipe
    z = np.load(os.path.join(GOLD, "loop_tiny_eta.npz"))
    usd, bsd = tiny_weights()
    steps = int(tag.split("_")[1])
    gs, ge = [float(v) for v in z[f"{tag}_window"]]
    eta, seed = float(z[f"{tag}_eta"]), int(z[f"{tag}_seed"])
    a = _loop_inputs()
    pipe = make_pipeline(usd, bsd, scheduler="ddim", use_graphs=graphs)
    # (i) teacher-forced per step: the oracle loop with the reference's noise, its latents fed to every GPU step
    ucfg, bcfg = tiny_cfgs()
    trace_ref = []
    noise_ref = torch.from_numpy(z[f"{tag}_noise"])
    o_pipe.denoise_loop(usd, ucfg, bsd, bcfg, _StochasticDDIMOracle(eta, noise_ref), steps, a["latents"], a["prompt"], a["fg"], a["bg"],
                        a["score"].float(), a["dino"], 7.5, 1.0, gs, ge, trace=trace_ref)
    np.testing.assert_allclose(trace_ref[1][1].numpy(), z[f"{tag}_eps"][1], rtol=1e-3, atol=1e-3)   # oracle == reference, past a noisy step
    trace = []
    pipe(a["prompt"], a["fg"], a["bg"], a["score"], a["dino"], num_inference_steps=steps, guidance_scale=7.5, latents=a["latents"],
         blobnet_control_guidance_start=gs, blobnet_control_guidance_end=ge, trace=trace, teacher_latents=[t[0] for t in trace_ref],
         eta=eta, generator=torch.Generator().manual_seed(seed))
    for i, ((eps_gpu, _), (_, eps_ref)) in enumerate(zip(trace, trace_ref)):
        e = rel_err(eps_gpu.cpu().numpy(), eps_ref.numpy())
        assert e < 1e-2, f"step {i}: guided eps rel err {e:.3e}"
        assert psnr(eps_gpu.cpu().numpy(), eps_ref.numpy()) > 40.0
    # (ii) free-running, the noise drawn by the engine from the same seed, against the reference's final latents
    out = pipe(a["prompt"], a["fg"], a["bg"], a["score"], a["dino"], num_inference_steps=steps, guidance_scale=7.5, latents=a["latents"],
               blobnet_control_guidance_start=gs, blobnet_control_guidance_end=ge, eta=eta,
               generator=torch.Generator().manual_seed(seed)).cpu().numpy()
    ref = z[f"{tag}_final"]
    print(f"{tag} eta {eta} graphs {graphs}: free-running final latents max-abs {np.abs(out - ref).max():.3e} "
          f"(|ref| max {np.abs(ref).max():.2f}), rel err {rel_err(out, ref):.3e}, PSNR {psnr(out, ref):.1f} dB")
    assert rel_err(out, ref) < 1e-2, f"free-running rel err {rel_err(out, ref):.3e}"
    assert psnr(out, ref) > 40.0
    # the same noise given as variance_noise gives the same latents, bit for bit
    out2 = pipe(a["prompt"], a["fg"], a["bg"], a["score"], a["dino"], num_inference_steps=steps, guidance_scale=7.5, latents=a["latents"],
                blobnet_control_guidance_start=gs, blobnet_control_guidance_end=ge, eta=eta, variance_noise=noise_ref).cpu().numpy()
    assert np.array_equal(out, out2)


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


def test_pipeline_call_with_eta_matches_the_reference_call(parts):
    from PIL import Image
    from blobctrl_amd.pipeline import StableDiffusionBlobNetPipeline
    from blobctrl_amd.schedulers import DDIMScheduler
    z = np.load(os.path.join(GOLD, "pipeline_call.npz"))
    ze = np.load(os.path.join(GOLD, "pipeline_call_eta.npz"))
    kw = dict(pipeline_cases()["ddim_neg2"])
    kw.pop("scheduler"), kw.pop("seed"), kw.pop("rng_seed")
    seed, rng_seed, eta = int(ze["seed"]), int(ze["rng_seed"]), float(ze["eta"])
    pipe = StableDiffusionBlobNetPipeline(tokenizer=FakeTokenizer(), scheduler=DDIMScheduler(), safety_checker=None,
                                          requires_safety_checker=False, **parts)
    drawn = []
    eng = pipe.engine

    def tapped(*a, **k):
        r = type(eng).variance_noise(*a, **k)
        drawn.append(r.detach().cpu().clone())
        return r
    eng.variance_noise = tapped
    common = dict(fg_image=Image.fromarray(z["fg"]), bg_image=Image.fromarray(z["bg"]), gs_score=torch.from_numpy(z["gs_score"]),
                  height=64, width=64, **kw)
    torch.manual_seed(rng_seed)                          # the VAE posterior samples come from the global generator, like pipe:304
    out = pipe(generator=torch.Generator().manual_seed(seed), eta=eta, output_type="latent", **common)
    got, ref = out.images.cpu().numpy(), ze["latents"]
    assert len(drawn) == 1 and np.array_equal(drawn[0].numpy(), ze["noise"]), "the engine drew other noise than the reference"
    rel = rel_err(got, ref)
    print(f"__call__ eta {eta}: end to end max-abs {np.abs(got - ref).max():.3e}, max-abs/scale {rel:.3e}, PSNR {psnr(got, ref):.1f} dB")
    assert got.shape == ref.shape and rel < 3e-2 and psnr(got, ref) > 36.0
    # the loop from the reference's own entry tensors, the generator continuing after the start latents as in the reference
    t = lambda k: torch.from_numpy(ze[f"entry_{k}"])
    B = t("prompt_embeds").shape[0]
    gen = torch.Generator().manual_seed(seed)
    noise = torch.randn((B, 4, 8, 8), generator=gen, dtype=torch.float32)
    got = eng.denoise(torch.cat([t("negative_prompt_embeds"), t("prompt_embeds")]), t("fg_latents"), t("bg_latents"),
                      torch.from_numpy(z["gs_score"]), t("dino"), num_inference_steps=kw["num_inference_steps"],
                      guidance_scale=float(kw["guidance_scale"]), latents=noise, blobnet_conditioning_scale=kw["blobnet_conditioning_scale"],
                      blobnet_control_guidance_start=kw["blobnet_control_guidance_start"],
                      blobnet_control_guidance_end=kw["blobnet_control_guidance_end"], eta=eta, generator=gen).cpu().numpy()
    r = rel_err(got, ref)
    print(f"__call__ eta {eta}: loop from the reference's entry tensors max-abs {np.abs(got - ref).max():.3e}, max-abs/scale {r:.3e}, "
          f"PSNR {psnr(got, ref):.1f} dB")
    assert r < 1e-2 and psnr(got, ref) > 40.0
    # UniPC has no eta (its step takes none): refused, with a message that points at DDIM
    from blobctrl_amd.schedulers import UniPCMultistepScheduler
    pipe.scheduler = UniPCMultistepScheduler()
    with pytest.raises(NotImplementedError, match="DDIM"):
        pipe(generator=torch.Generator().manual_seed(seed), eta=eta, output_type="latent", **common)


# ------------------------------------------------------------------------------------------------------------------ caches
def test_new_seeds_and_etas_replay_the_cached_plan_and_graph():
    usd, bsd = tiny_weights()
    a = _loop_inputs()
    eng = make_pipeline(usd, bsd, scheduler="ddim", use_graphs=True)
    run = lambda **kw: eng.denoise(a["prompt"], a["fg"], a["bg"], a["score"], a["dino"], num_inference_steps=5, latents=a["latents"],
                                   **kw).cpu()
    base = run()                                                         # eta = 0: its own (deterministic) plan
    x1 = run(eta=0.3, generator=torch.Generator().manual_seed(1))
    st = dict(eng.cache_stats)
    x1b = run(eta=0.3, generator=torch.Generator().manual_seed(1))
    assert torch.equal(x1, x1b)
    x2 = run(eta=0.3, generator=torch.Generator().manual_seed(2))
    x3 = run(eta=1.0, generator=torch.Generator().manual_seed(1))
    st2 = eng.cache_stats
    assert st2["plans_recorded"] == st["plans_recorded"] and st2["loop_graph_captures"] == st["loop_graph_captures"]
    assert st2["plan_hits"] == st["plan_hits"] + 3 and st2["loop_graph_hits"] == st["loop_graph_hits"] + 3
    assert not torch.equal(x1, x2) and not torch.equal(x1, x3) and not torch.equal(x1, base)
    assert torch.equal(base, run())                                      # eta = 0 is untouched by the stochastic plan next to it
    # the whole-edit graph and the eager launch list (a step-end callback forces the eager loop) apply the same noise
    eager = run(eta=1.0, generator=torch.Generator().manual_seed(1), callback_on_step_end=lambda *a_: {})
    r = rel_err(eager.numpy(), x3.numpy())
    print(f"graph vs eager (eta 1.0): max-abs/scale {r:.3e}")
    assert r < 1e-2 and psnr(eager.numpy(), x3.numpy()) > 40.0
    # generator=None: the global RNG of the engine's device
    torch.cuda.manual_seed(9)
    y1 = run(eta=1.0)
    torch.cuda.manual_seed(9)
    assert torch.equal(y1, run(eta=1.0))
    with pytest.raises(ValueError):
        run(eta=1.0, generator=torch.Generator(), variance_noise=torch.zeros(5, 1, 4, 8, 8))
    with pytest.raises(NotImplementedError):
        run(eta=-0.1)


def test_request_batch_with_one_generator_per_request():
    usd, bsd = tiny_weights()
    eng = make_pipeline(usd, bsd, scheduler="ddim", use_graphs=True)
    a = _loop_inputs()
    B, steps = 3, 5
    prompts = [g(60 + k, 2, 7, TINY["ctx"]) for k in range(B)]
    lat = [g(70 + k, 1, 4, 8, 8) for k in range(B)]
    fg = [a["fg"] * (1.0 + 0.1 * k) for k in range(B)]
    seeds = [101, 202, 303]
    singles = [eng.denoise(prompts[k], fg[k], a["bg"], a["score"], a["dino"], num_inference_steps=steps, latents=lat[k], eta=1.0,
                           generator=torch.Generator().manual_seed(seeds[k])).cpu().numpy() for k in range(B)]
    batch = eng.denoise(torch.cat([p[:1] for p in prompts] + [p[1:] for p in prompts]), torch.cat(fg), a["bg"].repeat(B, 1, 1, 1),
                        a["score"].repeat(B, 1, 1, 1), a["dino"].repeat(B, 1, 1), num_inference_steps=steps, latents=torch.cat(lat),
                        blobnet_conditioning_scale=[1.0] * B, eta=1.0,
                        generator=[torch.Generator().manual_seed(s) for s in seeds]).cpu().numpy()
    for k in range(B):
        r = rel_err(batch[k:k + 1], singles[k])
        print(f"request {k}: batch vs single edit max-abs/scale {r:.3e}, PSNR {psnr(batch[k:k + 1], singles[k]):.1f} dB")
        assert r < 1e-2 and psnr(batch[k:k + 1], singles[k]) > 40.0
    with pytest.raises(ValueError):
        eng.denoise(torch.cat([p[:1] for p in prompts] + [p[1:] for p in prompts]), torch.cat(fg), a["bg"].repeat(B, 1, 1, 1),
                    a["score"].repeat(B, 1, 1, 1), a["dino"].repeat(B, 1, 1), num_inference_steps=steps, latents=torch.cat(lat),
                    blobnet_conditioning_scale=[1.0] * B, eta=1.0, generator=[torch.Generator(), torch.Generator()])


# ------------------------------------------------------------------------------------------------------------------ full size
def test_fullsize_plan_indexes_the_noise_of_every_step():
    """The 512^2 batch-1 plan of the benchmark (conv_wreg, gemm256 and row-chain launches) with eta = 1 and a caller variance_noise,
    teacher-forced: every step's latents must be that step's OWN traced guided eps put through the eta = 1 row plus std * noise[step]
    (a wrong slice of the [50][1][4][64][64] buffer would show); with zero noise the latents differ by exactly std * noise."""
    import bench
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from blobctrl_amd.schedulers import DDIMTable
    from blobctrl_amd.splat import splat_features
    usd, bsd = bench.synth_weights()
    ucfg, bcfg = bench.full_configs()
    h = w = 64
    n = 50
    inp = bench.synth_inputs(h, w, batch=1)
    score = splat_features(**inp["blob"], score_size=(h, w), return_d_score=True, device="cuda:0")
    eng = BlobCtrlEngine(usd, bsd, ucfg, bcfg, device="cuda:0", scheduler="ddim")
    noise = g(4242, n, 1, 4, h, w)
    teach = [inp["latents"] * (1.0 - 0.01 * i) for i in range(n)]
    coef = DDIMTable().set_timesteps(n, eta=1.0).coef.double()

    def traced(vn):
        tr = []
        eng(inp["prompt"], inp["fg"], inp["bg"], score, inp["dino"], num_inference_steps=n, guidance_scale=7.5, latents=inp["latents"],
            blobnet_control_guidance_end=0.9, trace=tr, teacher_latents=teach, eta=1.0, variance_noise=vn)
        return [(e.cpu().double(), x.cpu().double()) for e, x in tr]

    tr = traced(noise)
    tr0 = traced(torch.zeros_like(noise))
    worst = worst0 = 0.0
    for i in range(n):
        c = coef[i]
        x = teach[i].double()
        e, got = tr[i]
        ref = c[8] * (x * c[0] - e * c[1]) + c[10] * e + c[12] * noise[i].double()
        err = (got - ref).abs().max().item() / got.abs().max().item()
        err0 = (got - c[12] * noise[i].double() - tr0[i][1]).abs().max().item() / got.abs().max().item()
        worst, worst0 = max(worst, err), max(worst0, err0)
        assert err <= 1e-5, (i, err)
        assert err0 <= 1e-5, (i, err0)
    print(f"512^2 eta 1: worst step arithmetic error {worst:.2e} of max |x|; zero-noise run differs by std * noise to {worst0:.2e}")


# ------------------------------------------------------------------------------------------------------------------ C host
def test_c_host_runs_the_stochastic_plan_file(tmp_path):
    """tools/make_plan_fixture.py --eta 1.0 compiles the 5-step stochastic edit of loop_tiny_eta.npz WITHOUT a GPU (the reference's
    noise embedded in the named buffer `variance_noise`); the unchanged plain-C host tests/c/plan_edit.c runs it eagerly, with per-step
    graphs and as one whole-edit graph, against the reference's final latents."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")          # the compile step must not need a GPU
    r = subprocess.run([sys.executable, os.path.join(repo, "tools", "make_plan_fixture.py"), str(tmp_path), "--eta", "1.0"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    exe = str(tmp_path / "plan_edit")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cc = subprocess.run(["gcc", "-O1", "-std=c11", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(repo, "include"), "-I", f"{rocm}/include",
                         os.path.join(repo, "tests", "c", "plan_edit.c"), "-o", exe, "-L", os.path.join(repo, "blobctrl_amd"),
                         "-lblobctrl_hip", "-L", f"{rocm}/lib", "-lamdhip64", "-lm",
                         f"-Wl,-rpath,{os.path.join(repo, 'blobctrl_amd')}", f"-Wl,-rpath,{rocm}/lib"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe, str(tmp_path / "tiny_edit.bcplan"), str(tmp_path / "tiny_edit_io.bin")], capture_output=True, text=True,
                         timeout=600)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert run.stdout.count("max-abs err") == 4 and "OK" in run.stdout
