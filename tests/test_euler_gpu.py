"""Euler, Euler-ancestral and Heun on MI355X: the scaled input assemblies (bc_assemble_input_scaled, bc_assemble_input_im2col_scaled)
against a plain torch expression of pipe:724-739 with the reference's division of the noisy latents, the step kernels on the new
tables, the tiny-net loop against the REFERENCE's own loops (tests/golden/loop_tiny_euler.npz), the reference pipeline's own `__call__`
(pipeline_call_euler.npz), the plan / graph caches when the scheduler changes between UniPC and Euler, and a compiled Euler plan
replayed by the plan runtime from a plain C host.

Bars (those of tests/test_dpm_solver_gpu.py for the same nets and recipe, fixed before measuring): assemblies bit for bit; step kernels
max-abs <= 1e-6 of max |ref| against an fp64 host evaluation and rtol / atol 2e-5 against the reference trajectory; tiny loop
(teacher-forced guided eps and free-running final latents) max-abs / scale < 1e-2 and PSNR > 40 dB; end-to-end __call__ < 3e-2 and
> 36 dB."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.common import PIPE, TINY, FakeTokenizer, g, pipeline_cases, psnr, tiny_pipeline_weights, tiny_weights  # noqa: E402
from tests.gpu_common import launch_step, make_pipeline, tiny_trunk_configs  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000, steps_offset=1)
DEV = "cuda:0"


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


def _same_timesteps(got, ref, karras):
    """Equal to the reference's, bit for bit.  One exception, measured: the FRACTIONAL timesteps of Karras sigmas (Euler and Heun do not
    round them) come out of `_sigma_to_t`, an interpolation in float32 log-sigmas, and numpy's float32 log is not the same function on
    every CPU.  The fixtures were written on an Intel Xeon; on an AMD EPYC 9575F 154 of the 1000 log-sigmas differ in the last bits and
    the reference itself would write other timesteps there: the tables then differ from the fixtures by 3.1e-5 (euler_trailing_karras_10,
    at t = 479.508), 1.2e-5 (heun_karras_6, t = 593.502) and 6.1e-5 (euler_karras_6, t = 593.502), one float32 ulp of the timestep.
    So: where this machine's log-sigmas ARE the fixture machine's (`train_log_sigmas` of schedulers_euler.npz), equality is required.
    Elsewhere the bar is 2e-4 of a timestep: one float32 ulp of log sigma (|log sigma| <= 2.7: 2.4e-7) at either end of an interval,
    over the flattest slope of the SD-1.5 schedule (3.27e-3 per timestep), is 1.5e-4, plus the float32 rounding of t itself (3e-5)."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.dtype != ref.dtype or got.shape != ref.shape:
        return False
    from blobctrl_amd.schedulers import _alphas_cumprod
    ac = _alphas_cumprod(1000, SD["beta_start"], SD["beta_end"])
    here = np.log((((1 - ac) / ac) ** 0.5).numpy())
    fixture_machine = np.array_equal(here, np.load(os.path.join(GOLD, "schedulers_euler.npz"))["train_log_sigmas"])
    if karras and not fixture_machine:
        return bool(np.abs(got.astype(np.float64) - ref).max() <= 2e-4)
    return np.array_equal(got, ref)


def _scheduler(cls, **kw):
    from blobctrl_amd import schedulers
    return {"euler": schedulers.EulerDiscreteScheduler, "euler_ancestral": schedulers.EulerAncestralDiscreteScheduler,
            "heun": schedulers.HeunDiscreteScheduler}[cls](**dict(SD, **kw))


# ------------------------------------------------------------------------------------------------------------------ assemblies
def _canvas(lat, img, score, feat, Bout, Cpad, dup, div):
    """pipe:724-739 (+ :706-721) on the CPU: [Bout][h][2w][Cpad] fp16 and the mask of the entries that hold noisy latents.  `div` (a
    0-dim fp32 tensor) divides the noisy latents in fp32 before the fp16 conversion; None = no scaling."""
    Blat, Bimg = lat.shape[0], img.shape[0]
    h, w = lat.shape[-2:]
    F = 0 if feat is None else feat.shape[1]
    X = torch.zeros(Bout, h, 2 * w, Cpad, dtype=torch.float16)
    noisy = torch.zeros(Bout, h, 2 * w, Cpad, dtype=torch.bool)
    x = lat if div is None else lat / div
    for b in range(Bout):
        bi = b % Bimg
        X[b, :, :w, :4] = img[bi].permute(1, 2, 0).half()
        X[b, :, w:, :4] = x[b % Blat].permute(1, 2, 0).half()
        noisy[b, :, w:, :4] = True
        sc = torch.cat([score[bi], score[bi]], 1)                              # the score under both halves
        X[b, :, :, 4] = sc.half()
        if F:
            X[b, :, :, 5:5 + F] = (sc[:, :, None] * feat[bi][None, None, :]).half()
        elif dup:
            X[b, :, :, 5] = sc.half()
    return X, noisy


def _im2col(X8):
    """[B][h][W][8] -> the 3x3 im2col operand [B][h * W][128]: k = tap * 8 + channel, zero outside the canvas and from k = 72."""
    B, h, W, _ = X8.shape
    pad = torch.zeros(B, h + 2, W + 2, 8, dtype=X8.dtype)
    pad[:, 1:-1, 1:-1] = X8
    out = torch.zeros(B, h, W, 128, dtype=X8.dtype)
    for t in range(9):
        out[..., t * 8:t * 8 + 8] = pad[:, t // 3:t // 3 + h, t % 3:t % 3 + W]
    return out.reshape(B, h * W, 128)


@pytest.mark.parametrize("F", [0, 11])
@pytest.mark.parametrize("Bout,Bimg", [(2, 1), (6, 1), (6, 3)])
@pytest.mark.parametrize("h,w", [(8, 8), (5, 7)])
def test_scaled_assemblies_divide_the_noisy_latents_and_nothing_else(h, w, Bout, Bimg, F):
    from blobctrl_amd import _lib
    from blobctrl_amd.schedulers import EulerDiscreteTable
    lib = _lib.load()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    Blat = Bout // 2
    nsteps = 10
    coef_host = EulerDiscreteTable().set_timesteps(nsteps).coef.clone()
    assert len(set(coef_host[:, 14].tolist())) == nsteps                       # the divisor differs by row
    coef = coef_host.to(DEV)
    lat = g(1, Blat, 4, h, w) * 9.0
    img, score = g(2, Bimg, 4, h, w), g(3, Bimg, h, w).abs()
    feat = g(4, Bimg, F) if F else None
    d_lat, d_img, d_score = lat.to(DEV), img.to(DEV), score.to(DEV)
    d_feat = feat.to(DEV) if F else None
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    Cpad = 8 if F == 0 else 16                                                  # F = 11: two 8-channel chunks

    def plain(scaled):
        X = torch.full((Bout, h, 2 * w, Cpad), 7.0, dtype=torch.float16, device=DEV)
        extra = (coef.data_ptr(), idx.data_ptr(), nsteps) if scaled else ()
        fn = lib.bc_assemble_input_scaled if scaled else lib.bc_assemble_input
        _lib.check(fn(d_lat.data_ptr(), Blat, d_img.data_ptr(), d_score.data_ptr(), d_feat.data_ptr() if F else None, Bimg, F, Bout, h, w,
                      Cpad, 0, *extra, X.data_ptr(), stream()), "assemble")
        torch.cuda.synchronize()
        return X.cpu()

    def im2col(scaled, dup):
        X = torch.full((Bout, h * 2 * w, 128), 7.0, dtype=torch.float16, device=DEV)
        extra = (coef.data_ptr(), idx.data_ptr(), nsteps) if scaled else ()
        fn = lib.bc_assemble_input_im2col_scaled if scaled else lib.bc_assemble_input_im2col
        _lib.check(fn(d_lat.data_ptr(), Blat, d_img.data_ptr(), d_score.data_ptr(), Bimg, Bout, h, w, dup, *extra, X.data_ptr(), stream()),
                   "assemble_im2col")
        torch.cuda.synchronize()
        return X.cpu()

    forms = [("plain", plain, lambda div: _canvas(lat, img, score, feat, Bout, Cpad, 0, div))]
    if F == 0:                                                                  # the im2col form has no feature channels
        for dup in (0, 1):
            def ref(div, dup=dup):
                X, noisy = _canvas(lat, img, score, None, Bout, 8, dup, div)
                return _im2col(X), _im2col(noisy)
            forms.append((f"im2col dup={dup}", lambda scaled, dup=dup: im2col(scaled, dup), ref))
    for what, run, ref in forms:
        unscaled = run(False)
        want0, noisy = ref(None)
        assert torch.equal(unscaled, want0), what                              # (the torch expression is the unscaled kernel's, to begin with)
        for step in (0, nsteps // 2, nsteps - 1):
            idx.fill_(step)
            got = run(True)
            want, _ = ref(coef_host[step, 14])
            # the clean latents, the score, the feature channels, the padding: what the unscaled entry point writes, bit for bit
            assert torch.equal(got[~noisy], unscaled[~noisy]), (what, step)
            if what == "plain":                                             # (said once more by name: left half, score, features)
                assert torch.equal(got[:, :, :w], unscaled[:, :, :w]) and torch.equal(got[..., 4], unscaled[..., 4]), (what, step)
                if F:
                    assert torch.equal(got[..., 5:], unscaled[..., 5:]) and got[..., 5:5 + F].abs().sum() > 0, (what, step)
            # the noisy latents: fp16(fp32(x) / c14), exactly
            assert torch.equal(got[noisy], want[noisy]) and torch.equal(got, want), (what, step)
            assert not torch.equal(got[noisy], unscaled[noisy]), (what, step)
        for step in (nsteps, nsteps + 2, -1):                                   # no table row: the unscaled kernel's output
            idx.fill_(step)
            assert torch.equal(run(True), unscaled), (what, step)
        assert int(idx.item()) == -1                                            # (the assemblies never advance the counter)


# ------------------------------------------------------------------------------------------------------------------ step kernels
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
@pytest.mark.parametrize("name", ["euler_trailing_karras_10", "heun_karras_6", "eulera_noise_15"])
def test_step_kernels_on_euler_tables(B, name):
    """The plain step on an Euler and on a Heun table (the corrector columns read `last` and `m0` written by the previous launch), the
    noise step on the Euler-ancestral table: against the schedulers_euler.npz trajectories (CFG 7.5 with a garbage left half) and the
    fp64 host row."""
    from blobctrl_amd import _lib
    from blobctrl_amd.schedulers import table_class
    lib = _lib.load()
    z = np.load(os.path.join(GOLD, "schedulers_euler.npz"))
    kw = json.loads(str(z[f"{name}_kw"]))
    cls, n_ = kw.pop("cls"), kw.pop("n")
    kw.pop("timesteps")
    Table = table_class(cls)
    tab = Table(**{k: v for k, v in dict(SD, **kw).items() if k != "beta_schedule" and (k != "steps_offset" or k in Table._option_defaults)})
    tab.set_timesteps(n_)
    form = "noise" if cls == "euler_ancestral" else "step"
    ref = z[f"{name}_traj"]
    nsteps = ref.shape[0] - 1
    assert nsteps == tab.coef.shape[0] and (cls != "heun" or bool((tab.coef[:, 2] != 0).any()))
    h = w = 8
    n = B * 4 * h * w
    coef = tab.coef.clone()
    coef[:, 11] = 7.5
    coef = coef.to(DEV)
    noise = torch.stack([g(200 + i, 1, 4, h, w).repeat(B, 1, 1, 1) for i in range(nsteps)]).to(DEV)
    x = torch.from_numpy(ref[0]).repeat(B, 1, 1, 1).to(DEV).contiguous()
    hist = torch.zeros(3, n, device=DEV)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    eps_out = torch.zeros(B, 4, h, w, device=DEV)
    worst = 0.0
    for i in range(nsteps):
        # eps token-major [2B][h][2w][4]: the right half holds uncond u and cond c with u + 7.5 (c - u) = the fixture's eps_i
        e = g(100 + i, 1, 4, h, w)[0].permute(1, 2, 0)
        u = g(300 + i, 1, h, w, 4)[0]
        tok = torch.randn(2 * B, h, 2 * w, 4, generator=torch.Generator().manual_seed(400 + i)) * 50     # garbage left half
        tok[:B, :, w:] = u
        tok[B:, :, w:] = u + (e - u) / 7.5
        tok = tok.to(DEV)
        x_in, hist_in = x.clone().cpu(), hist.clone().cpu()
        _lib.check(launch_step(lib, form, tok, x, coef, idx, hist, -1.0, B, h, w, eps_out, 1, noise=noise, nsteps=nsteps), form)
        torch.cuda.synchronize()
        xn, hist_ref, eh = _host_step(coef[i].cpu(), tok.cpu(), x_in, hist_in, noise[i].cpu() if form == "noise" else None, -1.0, B, h, w)
        for got, r_, what in ((x, xn, "latents"), (hist, hist_ref, "hist"), (eps_out, eh, "eps_out")):
            err = (got.cpu().double() - r_.reshape(got.shape)).abs().max().item()
            assert err <= 1e-6 * r_.abs().max().item(), (name, B, i, what, err)
        for b in range(B):                          # test_kernels_gpu.py:544: rtol 2e-5, atol 2e-5 * max |ref|
            got, r_ = x[b:b + 1].cpu().numpy().astype(np.float64), ref[i + 1].astype(np.float64)
            worst = max(worst, rel_err(got, r_))
            assert (np.abs(got - r_) <= 2e-5 * np.abs(r_) + 2e-5 * np.abs(r_).max()).all(), (name, B, i, b, rel_err(got, r_))
    assert int(idx.item()) == nsteps
    print(f"{form} B={B} ({name}): worst per-step rel err vs the reference trajectory {worst:.2e}")


# ------------------------------------------------------------------------------------------------------------------ tiny loop
def _loop_inputs():
    from oracle import blob_splat
    score = torch.from_numpy(blob_splat.splat_scores_from_ellipse([[40.0, 42.0], [20.0, 30.0], 25.0], 64, 64, 8, 8))
    return dict(latents=g(31, 1, 4, 8, 8), prompt=g(32, 2, 7, TINY["ctx"]), fg=g(33, 1, 4, 8, 8) * 0.18215 * 5,
                bg=g(34, 1, 4, 8, 8) * 0.18215 * 5, score=score, dino=g(35, 1, 1, TINY["feat"]))


def _use(eng, cls, **kw):
    s = _scheduler(cls, **kw)
    eng.set_scheduler(s.kind, s.table_params())
    return s


@pytest.mark.parametrize("tag", ["euler_leading_6", "euler_linspace_5", "euler_karras_6", "eulera_5", "heun_4", "euler_custom_8"])
@pytest.mark.parametrize("graphs", [False, True])
def test_euler_loop_matches_the_reference(tag, graphs):
    z = np.load(os.path.join(GOLD, "loop_tiny_euler.npz"))
    usd, bsd = tiny_weights()
    kw = json.loads(str(z[f"{tag}_kw"]))
    cls, steps, ts = kw.pop("cls"), kw.pop("n"), kw.pop("timesteps")
    gs, ge = [float(v) for v in z[f"{tag}_window"]]
    seeded = f"{tag}_noise" in z.files
    a = _loop_inputs()
    eng = make_pipeline(usd, bsd, scheduler="unipc", use_graphs=graphs)
    _use(eng, cls, **kw)
    extra = dict(timesteps=ts) if ts is not None else dict(num_inference_steps=steps)
    gen = (lambda: torch.Generator().manual_seed(int(z[f"{tag}_seed"]))) if seeded else (lambda: None)
    run = lambda **k: eng.denoise(a["prompt"], a["fg"], a["bg"], a["score"], a["dino"], guidance_scale=7.5, latents=a["latents"],
                                  blobnet_control_guidance_start=gs, blobnet_control_guidance_end=ge, **extra, **k)
    # (i) teacher-forced: the reference's latents (in its sigma space) entering every step, its guided eps out
    trace = []
    run(trace=trace, teacher_latents=[torch.from_numpy(v) for v in z[f"{tag}_lat"]], generator=gen())
    assert _same_timesteps(eng.timesteps.numpy(), z[f"{tag}_timesteps"], kw.get("use_karras_sigmas"))
    assert len(trace) == len(z[f"{tag}_eps"]) == (2 * steps - 1 if cls == "heun" else len(z[f"{tag}_timesteps"]))
    for i, (eps_gpu, _) in enumerate(trace):
        ref = z[f"{tag}_eps"][i]
        e = rel_err(eps_gpu.cpu().numpy(), ref)
        print(f"{tag} step {i}: teacher-forced guided eps rel err {e:.3e}, PSNR {psnr(eps_gpu.cpu().numpy(), ref):.1f} dB")
        assert e < 1e-2 and psnr(eps_gpu.cpu().numpy(), ref) > 40.0, f"step {i}: guided eps rel err {e:.3e}"
    # (ii) free-running against the reference's final latents
    out = run(generator=gen()).cpu().numpy()
    ref = z[f"{tag}_final"]
    print(f"{tag} graphs {graphs}: free-running final latents rel err {rel_err(out, ref):.3e}, PSNR {psnr(out, ref):.1f} dB")
    assert rel_err(out, ref) < 1e-2 and psnr(out, ref) > 40.0
    if seeded:                                      # the tapped noise as variance_noise: bit-identical to the generator run
        out2 = run(variance_noise=torch.from_numpy(z[f"{tag}_noise"])).cpu().numpy()
        assert np.array_equal(out, out2)


def test_engine_refusals_for_the_new_schedulers():
    usd, bsd = tiny_weights()
    a = _loop_inputs()
    eng = make_pipeline(usd, bsd, scheduler="unipc", use_graphs=False)
    run = lambda **k: eng.denoise(a["prompt"], a["fg"], a["bg"], a["score"], a["dino"], guidance_scale=7.5, latents=a["latents"], **k)
    _use(eng, "euler")
    with pytest.raises(NotImplementedError, match="eta"):
        run(num_inference_steps=4, eta=0.5)
    with pytest.raises(ValueError, match="variance_noise"):
        run(num_inference_steps=4, variance_noise=torch.zeros(4, 1, 4, 8, 8))
    for cls in ("heun", "euler_ancestral"):
        _use(eng, cls)
        with pytest.raises(NotImplementedError, match="timesteps"):
            run(timesteps=[999, 700, 400, 20])
        with pytest.raises(NotImplementedError, match="eta"):
            run(num_inference_steps=4, eta=0.5)
    assert eng.cache_stats["plans_recorded"] == 0                               # every refusal comes before a plan is recorded


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


def test_pipeline_call_with_euler_schedulers_matches_the_reference_call(parts):
    from PIL import Image
    from blobctrl_amd.pipeline import StableDiffusionBlobNetPipeline
    from blobctrl_amd.schedulers import (DDIMScheduler, EulerAncestralDiscreteScheduler, EulerDiscreteScheduler, HeunDiscreteScheduler)
    z = np.load(os.path.join(GOLD, "pipeline_call.npz"))
    ze = np.load(os.path.join(GOLD, "pipeline_call_euler.npz"))
    kw = dict(pipeline_cases()["ddim_neg2"])
    for k in ("scheduler", "seed", "rng_seed", "num_inference_steps"):
        kw.pop(k)
    seed, rng_seed, steps = int(ze["seed"]), int(ze["rng_seed"]), int(ze["num_inference_steps"])
    pipe = StableDiffusionBlobNetPipeline(tokenizer=FakeTokenizer(), scheduler=DDIMScheduler(**SD), safety_checker=None,
                                          requires_safety_checker=False, **parts)
    common = dict(fg_image=Image.fromarray(z["fg"]), bg_image=Image.fromarray(z["bg"]), gs_score=torch.from_numpy(z["gs_score"]),
                  height=64, width=64, output_type="latent", **kw)
    src = pipe.scheduler.config
    for tag, sch in (("euler", EulerDiscreteScheduler.from_config(src)),
                     ("eulera", EulerAncestralDiscreteScheduler.from_config(src, timestep_spacing="leading"))):
        pipe.scheduler = sch
        torch.manual_seed(rng_seed)
        out = pipe(num_inference_steps=steps, generator=torch.Generator().manual_seed(seed), **common)
        got, ref = out.images.cpu().numpy(), ze[f"{tag}_latents"]
        assert pipe.num_timesteps == steps and np.array_equal(pipe.scheduler.timesteps.cpu().numpy(), ze[f"{tag}_timesteps"])
        rel = rel_err(got, ref)
        print(f"__call__ {tag} on {ze[f'{tag}_timesteps']}: end to end max-abs/scale {rel:.3e}, PSNR {psnr(got, ref):.1f} dB")
        assert got.shape == ref.shape and rel < 3e-2 and psnr(got, ref) > 36.0
    assert ze["euler_timesteps"][1] != round(float(ze["euler_timesteps"][1]))   # (the Euler call ran on fractional timesteps)
    # caller timesteps: Euler takes them, Heun and Euler-ancestral refuse; eta is refused by all three
    pipe.scheduler = EulerDiscreteScheduler.from_config(src)
    out = pipe(timesteps=[999, 600, 200], generator=torch.Generator().manual_seed(seed), **common)
    assert pipe.num_timesteps == 3 and pipe.scheduler.timesteps.tolist() == [999.0, 600.0, 200.0] and torch.isfinite(out.images).all()
    with pytest.raises(NotImplementedError, match="eta"):
        pipe(num_inference_steps=steps, eta=0.5, generator=torch.Generator().manual_seed(seed), **common)
    for sch in (HeunDiscreteScheduler.from_config(src), EulerAncestralDiscreteScheduler.from_config(src)):
        pipe.scheduler = sch
        with pytest.raises(NotImplementedError, match="timesteps"):
            pipe(timesteps=[999, 600, 200], generator=torch.Generator().manual_seed(seed), **common)


# ------------------------------------------------------------------------------------------------------------------ caches
def test_unipc_euler_unipc_keep_their_own_plans_and_each_matches_its_reference():
    usd, bsd = tiny_weights()
    a = _loop_inputs()
    zl = np.load(os.path.join(GOLD, "loop_tiny.npz"))
    ze = np.load(os.path.join(GOLD, "loop_tiny_euler.npz"))
    eng = make_pipeline(usd, bsd, scheduler="unipc", use_graphs=True)
    from blobctrl_amd.schedulers import UniPCMultistepScheduler
    u = UniPCMultistepScheduler()
    run = lambda ge: eng.denoise(a["prompt"], a["fg"], a["bg"], a["score"], a["dino"], num_inference_steps=6, guidance_scale=7.5,
                                 latents=a["latents"], blobnet_control_guidance_start=0.0, blobnet_control_guidance_end=ge).cpu().numpy()
    eng.set_scheduler(u.kind, u.table_params())
    x_u = run(0.67)
    st = dict(eng.cache_stats)
    _use(eng, "euler", use_karras_sigmas=True)
    x_e = run(0.67)
    st1 = dict(eng.cache_stats)
    # Euler never replays UniPC's launches: a plan and a whole-edit graph of its own, same geometry and same active / inactive pattern
    assert st1["plans_recorded"] == st["plans_recorded"] + 1 and st1["loop_graph_captures"] == st["loop_graph_captures"] + 1
    assert st1["plan_hits"] == st["plan_hits"] and st1["loop_graph_hits"] == st["loop_graph_hits"]
    eng.set_scheduler(u.kind, u.table_params())
    x_u2 = run(0.67)
    _use(eng, "euler", use_karras_sigmas=True)
    x_e2 = run(0.67)
    st2 = eng.cache_stats
    assert st2["plans_recorded"] == st1["plans_recorded"] and st2["loop_graph_captures"] == st1["loop_graph_captures"]
    assert st2["plan_hits"] == st1["plan_hits"] + 2 and st2["loop_graph_hits"] == st1["loop_graph_hits"] + 2
    for got, ref, what in ((x_u, zl["unipc_6_final"], "unipc"), (x_e, ze["euler_karras_6_final"], "euler karras"),
                           (x_u2, zl["unipc_6_final"], "unipc again"), (x_e2, ze["euler_karras_6_final"], "euler karras again")):
        print(f"{what}: rel err {rel_err(got, ref):.3e}, PSNR {psnr(got, ref):.1f} dB")
        assert rel_err(got, ref) < 1e-2 and psnr(got, ref) > 40.0, what
    assert np.array_equal(x_u, x_u2) and np.array_equal(x_e, x_e2)


# ------------------------------------------------------------------------------------------------------------------ plan runtime
def test_c_host_replays_a_compiled_euler_plan_to_the_engines_latents(tmp_path):
    """tools/make_plan_fixture.py compiles the Euler edit WITHOUT a GPU; tests/c/plan_edit.c loads it with bc_plan_load and runs it
    eagerly, with per-step graphs and as one whole-loop graph: each must land on what the in-process engine computed for the same edit
    (plan_edit's own bar: 1e-2 of scale)."""
    z = np.load(os.path.join(GOLD, "loop_tiny_euler.npz"))
    tag = "euler_leading_6"
    usd, bsd = tiny_weights()
    a = _loop_inputs()
    eng = make_pipeline(usd, bsd, scheduler="unipc", use_graphs=False)
    _use(eng, "euler", timestep_spacing="leading")
    gs, ge = [float(v) for v in z[f"{tag}_window"]]
    mine = eng.denoise(a["prompt"], a["fg"], a["bg"], a["score"], a["dino"], num_inference_steps=6, guidance_scale=7.5, latents=a["latents"],
                       blobnet_control_guidance_start=gs, blobnet_control_guidance_end=ge).cpu().numpy()
    assert rel_err(mine, z[f"{tag}_final"]) < 1e-2
    np.save(tmp_path / "expected.npy", mine)
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")          # the compile step must not need a GPU
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "make_plan_fixture.py"), str(tmp_path), "--euler", tag, "--expected",
                        str(tmp_path / "expected.npy")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    exe = str(tmp_path / "plan_edit")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cc = subprocess.run(["gcc", "-O1", "-std=c11", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(REPO, "include"), "-I", f"{rocm}/include",
                         os.path.join(REPO, "tests", "c", "plan_edit.c"), "-o", exe, "-L", os.path.join(REPO, "blobctrl_amd"),
                         "-lblobctrl_hip", "-L", f"{rocm}/lib", "-lamdhip64", "-lm",
                         f"-Wl,-rpath,{os.path.join(REPO, 'blobctrl_amd')}", f"-Wl,-rpath,{rocm}/lib"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe, str(tmp_path / "tiny_edit.bcplan"), str(tmp_path / "tiny_edit_io.bin")], capture_output=True, text=True,
                         timeout=600)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert run.stdout.count("max-abs err") == 4 and "OK" in run.stdout
