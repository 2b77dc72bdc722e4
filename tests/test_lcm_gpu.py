"""LCM few-step edits on MI355X: the single-pass step (bc_scheduler_step_single) in its plain / noise / third-order forms against an
fp64 host row and the reference trajectories, the tiny-net loops against the REFERENCE's own loops (tests/golden/loop_tiny_lcm.npz: LCM
with and without guidance, guidance-free DDIM and UniPC), the reference pipeline's own `__call__` (pipeline_call_lcm.npz), the plan /
graph caches when the scheduler changes between UniPC and LCM, and a compiled single-pass plan replayed by the plan runtime from a plain
C host.

Bars (those of tests/test_euler_gpu.py for the same nets and recipe, fixed before measuring): step kernels max-abs <= 1e-6 of max |ref|
against an fp64 host evaluation and rtol / atol 2e-5 against the reference trajectory; tiny loop (teacher-forced eps and free-running
final latents) max-abs / scale < 1e-2 and PSNR > 40 dB; end-to-end __call__ < 3e-2 and > 36 dB."""
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
from tests.gpu_common import make_pipeline, tiny_trunk_configs  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000, steps_offset=1)
DEV = "cuda:0"


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------------------------ time embedding
COND_DIM = 8


def _cond_unet():
    """(state dict, TrunkConfig) of the tiny UNet with time_cond_proj_dim = 8: the plain tiny UNet plus time_embedding.cond_proj.weight."""
    import dataclasses
    from blobctrl_amd import synth
    c = TINY
    shapes = synth.trunk_param_shapes(5, c["boc"], 2, c["ctx"], 4, blobnet=False, time_cond_proj_dim=COND_DIM)
    return synth.synth_state_dict(shapes, c["seed"]), dataclasses.replace(tiny_trunk_configs()[0], time_cond_proj_dim=COND_DIM)


def _cond_engine(graphs=True):
    from blobctrl_amd.pipeline import BlobCtrlEngine
    usd, ucfg = _cond_unet()
    return BlobCtrlEngine(usd, tiny_weights()[1], ucfg, tiny_trunk_configs()[1], device=DEV, scheduler="unipc", use_graphs=graphs)


@pytest.mark.parametrize("nsteps", [1, 4])
@pytest.mark.parametrize("dim", [16, 320])
@pytest.mark.parametrize("rows_per_step", [1, 3])
def test_cond_time_embedding_is_the_fp64_sum_rounded_once(rows_per_step, dim, nsteps):
    """bc_timestep_embedding_table_cond / bc_timestep_embedding_cond against [cos | sin](t * exp(-ln 1e4 * k / half)) + cond evaluated in
    fp64 on the host and rounded ONCE to fp16: equal.  (Rounding the sinusoid to fp16 first and adding then would differ in the last
    bit of about every third entry; so would a cond row taken from another image.)  The old entry points give what they gave."""
    from blobctrl_amd import _lib
    lib = _lib.load()
    ts = torch.tensor([999.0, 759.0, 499.5, 19.0][:nsteps])
    cond = g(7, rows_per_step, dim) * 0.7
    half = dim // 2
    k = np.arange(half, dtype=np.float64)
    freq = np.exp(-np.log(10000.0) * k / half)

    def host(tvals, cond_rows):
        a = np.asarray(tvals, np.float64)[:, None] * freq[None, :]
        v = np.concatenate([np.cos(a), np.sin(a)], 1) + cond_rows.double().numpy()
        return torch.from_numpy(v).to(torch.float16)

    d_t, d_cond = ts.to(DEV), cond.to(DEV)
    rows = nsteps * rows_per_step
    out = torch.full((rows + 1, dim), 7.0, dtype=torch.float16, device=DEV)          # (one row more: nothing is written past the end)
    _lib.check(lib.bc_timestep_embedding_table_cond(d_t.data_ptr(), nsteps, rows_per_step, dim, d_cond.data_ptr(), out.data_ptr(), _stream()),
               "bc_timestep_embedding_table_cond")
    plain = torch.full((rows + 1, dim), 7.0, dtype=torch.float16, device=DEV)
    _lib.check(lib.bc_timestep_embedding_table(d_t.data_ptr(), nsteps, rows_per_step, dim, plain.data_ptr(), _stream()), "table")
    torch.cuda.synchronize()
    want = host(ts.repeat_interleave(rows_per_step).tolist(), cond.repeat(nsteps, 1))
    assert torch.equal(out[:rows].cpu(), want) and (out[rows] == 7.0).all() and (plain[rows] == 7.0).all()
    twice = (plain[:rows].cpu().float() + cond.repeat(nsteps, 1)).half()               # what rounding twice would give
    print(f"rows_per_step {rows_per_step} dim {dim} steps {nsteps}: {(twice != want).float().mean():.3f} of the entries differ when rounded twice")
    assert rows_per_step == 1 or not torch.equal(out[:rows].cpu(), host(ts.repeat_interleave(rows_per_step).tolist(),
                                                                          cond.roll(1, 0).repeat(nsteps, 1)))
    # per-step form: t through the device index, through t_value, rows identical in t and each with its own cond row
    idx = torch.tensor([nsteps - 1], dtype=torch.int32, device=DEV)
    for t_table, t_idx, t_value, t in ((d_t.data_ptr(), idx.data_ptr(), 0.0, float(ts[nsteps - 1])), (None, None, 981.0, 981.0)):
        one = torch.full((rows_per_step + 1, dim), 7.0, dtype=torch.float16, device=DEV)
        old = torch.full((rows_per_step + 1, dim), 7.0, dtype=torch.float16, device=DEV)
        _lib.check(lib.bc_timestep_embedding_cond(t_table, t_idx, t_value, rows_per_step, dim, d_cond.data_ptr(), one.data_ptr(), _stream()),
                   "bc_timestep_embedding_cond")
        _lib.check(lib.bc_timestep_embedding(t_table, t_idx, t_value, rows_per_step, dim, old.data_ptr(), _stream()), "bc_timestep_embedding")
        torch.cuda.synchronize()
        assert torch.equal(one[:rows_per_step].cpu(), host([t] * rows_per_step, cond)) and (one[rows_per_step] == 7.0).all()
        # the old entry points: the fp32 kernel's output, as tests/test_kernels_gpu.py bounds it, and the same from both of them
        from oracle.nets import timestep_embedding
        ref = timestep_embedding(torch.tensor([t] * rows_per_step), dim)
        assert (old[:rows_per_step].cpu().float() - ref).abs().max() <= 2e-3
        if t_table is not None:
            assert torch.equal(old[:rows_per_step], plain[rows - rows_per_step:rows])
    with pytest.raises(_lib.BlobCtrlHipError):
        _lib.check(lib.bc_timestep_embedding_table_cond(d_t.data_ptr(), nsteps, rows_per_step, dim, None, out.data_ptr(), _stream()), "null cond")


def test_time_cond_unet_module_honours_timestep_cond():
    """The module shell on the reference's forward of the tiny UNet with time_cond_proj_dim = 8 (unet_tiny_timecond.npz; the bar
    tests/test_parity_gpu.py holds the tiny UNet to: max-abs / scale < 1e-2, PSNR > 40 dB): with a timestep_cond (one embedding per
    image), with BlobNet residuals and without, and with none at all (no add)."""
    from blobctrl_amd.modules import UNet2DConditionModel
    z = np.load(os.path.join(GOLD, "unet_tiny_timecond.npz"))
    usd, ucfg = _cond_unet()
    unet = UNet2DConditionModel(usd, ucfg)
    assert unet.config.time_cond_proj_dim == COND_DIM
    x, ehs, tc = (torch.from_numpy(z[k]).to(DEV) for k in ("unet_in", "ehs", "timestep_cond"))
    t = int(z["timestep"])
    res = lambda: dict(down_block_add_samples=[torch.from_numpy(z[f"down_{i}"]).to(DEV) for i in range(12)],
                       mid_block_add_sample=torch.from_numpy(z["mid"]).to(DEV),
                       up_block_add_samples=[torch.from_numpy(z[f"up_{i}"]).to(DEV) for i in range(15)])
    for what, kw, ref in (("cond + residuals", dict(timestep_cond=tc, **res()), z["eps"]), ("cond", dict(timestep_cond=tc), z["eps_plain"]),
                          ("no cond", res(), z["eps_nocond"])):
        got = unet(x, t, encoder_hidden_states=ehs, return_dict=False, **kw)[0].cpu().numpy()
        print(f"time-cond UNet, {what}: rel {rel_err(got, ref):.3e}, PSNR {psnr(got, ref):.1f} dB")
        assert rel_err(got, ref) < 1e-2 and psnr(got, ref) > 40.0, what
    assert rel_err(z["eps"], z["eps_nocond"]) > 0.1                    # (the condition matters: the three references are far apart)
    swapped = unet(x, t, encoder_hidden_states=ehs, timestep_cond=tc.flip(0), return_dict=False)[0].cpu().numpy()
    assert rel_err(swapped, z["eps_plain"]) > 1e-2                      # ... and per image
    assert sorted(len(k) for k in unet._plans) == [6, 7, 7]             # calls without a timestep_cond keep the plan key they had
    with pytest.raises(ValueError, match="timestep_cond"):
        unet(x, t, encoder_hidden_states=ehs, timestep_cond=tc[:1], return_dict=False)
    plain = UNet2DConditionModel(tiny_weights()[0], tiny_trunk_configs()[0])
    with pytest.raises(ValueError, match="cond_proj"):
        plain(x, t, encoder_hidden_states=ehs, timestep_cond=tc, return_dict=False)
    assert plain.config.time_cond_proj_dim is None and not plain._plans


# ------------------------------------------------------------------------------------------------------------------ step kernel
def _host_step(c, e, x, hist, noise, third):
    """fp64: one table row on eps `e` [B, 4, h, w] (+ c12 * noise, + c13 * x0_{i-2})."""
    c = c.double()
    B = x.shape[0]
    n = x.numel()
    m0, m1, last = (hist.double()[k].reshape(x.shape) for k in range(3))
    xd, e = x.double(), e.double()
    x0 = xd * c[0] - e * c[1]
    xc = c[3] * last + c[4] * m0 + c[5] * m1 + c[6] * x0 if c[2] != 0 else xd
    xn = c[7] * xc + c[8] * x0 + c[9] * m0 + c[10] * e
    if third:
        xn = xn + c[13] * m1
    if noise is not None:
        xn = xn + c[12] * noise.double()
    return xn, torch.stack([x0.reshape(n), m0.reshape(n), xc.reshape(n)])


def _tables():
    """(name, table, reference trajectory or None, eps seed base, noise?, third?)"""
    from blobctrl_amd.schedulers import DDIMTable, DPMSolverMultistepTable, LCMTable, UniPCTable
    zl = np.load(os.path.join(GOLD, "schedulers_lcm.npz"))
    z = np.load(os.path.join(GOLD, "schedulers.npz"))
    zd = np.load(os.path.join(GOLD, "schedulers_dpm.npz"))
    return {
        "lcm_4": (LCMTable(set_alpha_to_one=False).set_timesteps(4), zl["lcm_4_traj"], True, False),
        "lcm_8": (LCMTable(set_alpha_to_one=False).set_timesteps(8), zl["lcm_8_traj"], True, False),
        "lcm_custom_4": (LCMTable(set_alpha_to_one=False).set_timesteps(timesteps=[939, 601, 320, 19]), zl["lcm_custom_4_traj"], True, False),
        "ddim_5": (DDIMTable().set_timesteps(5), z["ddim_5_traj"], False, False),
        "unipc_5": (UniPCTable().set_timesteps(5), z["unipc_5_traj"], False, False),
        "dpm3_14": (DPMSolverMultistepTable(solver_order=3).set_timesteps(14), zd["pp3_lin_14_traj"], False, True),
    }


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", ["lcm_4", "lcm_8", "lcm_custom_4", "ddim_5", "unipc_5", "dpm3_14"])
def test_single_pass_step_on_lcm_ddim_unipc_and_third_order_rows(B, name):
    """bc_scheduler_step_single: eps [B][h][2w][4], e = the right half of image b.  The eps buffer is allocated as a CFG layout would be
    (2B images) with NaN in the rows a single-pass layout does not have, and garbage in every left half: reading image B + b, or
    blending anything into e, shows as NaN or a wrong number.  An out-of-range step index leaves every buffer untouched."""
    from blobctrl_amd import _lib
    lib = _lib.load()
    tab, ref, noisy, third = _tables()[name]
    coef_host = tab.coef.clone()
    coef_host[:, 11] = 7.5                                            # (a guidance scale in the table must not be read)
    nsteps = coef_host.shape[0]
    assert (not third) or bool((coef_host[:, 13] != 0).any())
    assert ref.shape[0] == nsteps + 1
    h = w = 8
    n = B * 4 * h * w
    coef = coef_host.to(DEV)
    noise = torch.stack([g(200 + i, 1, 4, h, w).repeat(B, 1, 1, 1) for i in range(nsteps)]).to(DEV)
    x = torch.from_numpy(ref[0]).repeat(B, 1, 1, 1).to(DEV).contiguous()
    hist = torch.zeros(3, n, device=DEV)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    eps_out = torch.zeros(B, 4, h, w, device=DEV)
    step = lambda tok, adv=1: _lib.check(lib.bc_scheduler_step_single(
        tok.data_ptr(), x.data_ptr(), coef.data_ptr(), idx.data_ptr(), hist.data_ptr(), B, h, w, noise.data_ptr() if noisy else None, nsteps,
        int(third), eps_out.data_ptr(), adv, _stream()), "bc_scheduler_step_single")
    worst = 0.0
    for i in range(nsteps):
        e = g(100 + i, 1, 4, h, w).repeat(B, 1, 1, 1)
        tok = torch.randn(2 * B, h, 2 * w, 4, generator=torch.Generator().manual_seed(400 + i)) * 50      # garbage left halves
        tok[:B, :, w:] = e.permute(0, 2, 3, 1)
        tok[B:] = float("nan")                                         # what a CFG layout would hold there
        tok = tok.to(DEV)
        x_in, hist_in = x.clone().cpu(), hist.clone().cpu()
        step(tok)
        torch.cuda.synchronize()
        xn, hist_ref = _host_step(coef_host[i], e, x_in, hist_in, noise[i].cpu() if noisy else None, third)
        for got, r_, what in ((x, xn, "latents"), (hist, hist_ref, "hist"), (eps_out, e.double(), "eps_out")):
            assert torch.isfinite(got).all(), (name, B, i, what)
            err = (got.cpu().double() - r_.reshape(got.shape)).abs().max().item()
            assert err <= 1e-6 * r_.abs().max().item(), (name, B, i, what, err)
        for b in range(B):                          # tests/test_kernels_gpu.py: rtol 2e-5, atol 2e-5 * max |ref|
            got, r_ = x[b:b + 1].cpu().numpy().astype(np.float64), ref[i + 1].astype(np.float64)
            worst = max(worst, rel_err(got, r_))
            assert (np.abs(got - r_) <= 2e-5 * np.abs(r_) + 2e-5 * np.abs(r_).max()).all(), (name, B, i, b, rel_err(got, r_))
    assert int(idx.item()) == nsteps
    print(f"single-pass step B={B} ({name}): worst per-step rel err vs the reference trajectory {worst:.2e}")
    # no table row for this index (the counter stands at nsteps; then -1): nothing is written, the counter still advances when asked
    before = [t.clone() for t in (x, hist, eps_out)]
    tok = (torch.randn(2 * B, h, 2 * w, 4, generator=torch.Generator().manual_seed(9)) * 50).to(DEV)
    step(tok, 0)
    idx.fill_(-1)
    step(tok, 1)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (x, hist, eps_out))) and int(idx.item()) == 0


# ------------------------------------------------------------------------------------------------------------------ tiny loop
def _loop_inputs():
    from oracle import blob_splat
    score = torch.from_numpy(blob_splat.splat_scores_from_ellipse([[40.0, 42.0], [20.0, 30.0], 25.0], 64, 64, 8, 8))
    return dict(latents=g(31, 1, 4, 8, 8), prompt=g(32, 2, 7, TINY["ctx"]), fg=g(33, 1, 4, 8, 8) * 0.18215 * 5,
                bg=g(34, 1, 4, 8, 8) * 0.18215 * 5, score=score, dino=g(35, 1, 1, TINY["feat"]))


def _scheduler(cls):
    from blobctrl_amd import schedulers
    src = schedulers.DDIMScheduler(**SD).config
    return {"lcm": schedulers.LCMScheduler, "ddim": schedulers.DDIMScheduler, "unipc": schedulers.UniPCMultistepScheduler}[cls].from_config(src)


def _use(eng, cls):
    s = _scheduler(cls)
    eng.set_scheduler(s.kind, s.table_params())
    return s


def _run_case(eng, z, tag, a, **over):
    """(run(**kw) -> final latents tensor, the case's keyword record): the engine call of a loop_tiny_lcm.npz case."""
    from blobctrl_amd.pipeline import get_guidance_scale_embedding
    kw = json.loads(str(z[f"{tag}_kw"]))
    _use(eng, kw["cls"])
    gs, ge = [float(v) for v in z[f"{tag}_window"]]
    guidance, B, wcond = float(kw["guidance_scale"]), int(kw["batch"]), kw["time_cond_proj_dim"] is not None
    cfg = guidance > 1.0 and not wcond                                  # pipe:497
    prompt = g(32, 2 * B, 7, TINY["ctx"])
    prompt = prompt if cfg else prompt[B:]                              # guidance off: the positive prompts only, as the reference holds them
    call = dict(guidance_scale=guidance, latents=g(31, B, 4, 8, 8), blobnet_control_guidance_start=gs, blobnet_control_guidance_end=ge,
                do_classifier_free_guidance=cfg, **kw["set_timesteps"])
    if wcond:                                                           # pipe:987-993
        call["timestep_cond"] = get_guidance_scale_embedding(torch.full((B,), guidance - 1), kw["time_cond_proj_dim"])
        assert np.array_equal(call["timestep_cond"].numpy(), z[f"{tag}_timestep_cond"])
    call.update(over)
    return (lambda **k: eng.denoise(prompt, a["fg"], a["bg"], a["score"], a["dino"], **dict(call, **k))), kw


def _check_case(eng, z, tag, a, graphs, **over):
    run, kw = _run_case(eng, z, tag, a, **over)
    seeded = f"{tag}_noise" in z.files
    gen = (lambda: torch.Generator().manual_seed(int(z[f"{tag}_seed"]))) if seeded else (lambda: None)
    # (i) teacher-forced: the reference's latents entering every step, its (guided) eps out
    trace = []
    run(trace=trace, teacher_latents=[torch.from_numpy(v) for v in z[f"{tag}_lat"]], generator=gen())
    assert np.array_equal(eng.timesteps.numpy(), z[f"{tag}_timesteps"]) and len(trace) == len(z[f"{tag}_eps"])
    for i, (eps_gpu, _) in enumerate(trace):
        ref = z[f"{tag}_eps"][i]
        e = rel_err(eps_gpu.cpu().numpy(), ref)
        print(f"{tag} step {i}: teacher-forced eps rel err {e:.3e}, PSNR {psnr(eps_gpu.cpu().numpy(), ref):.1f} dB")
        assert e < 1e-2 and psnr(eps_gpu.cpu().numpy(), ref) > 40.0, f"step {i}: eps rel err {e:.3e}"
    # (ii) free-running against the reference's final latents
    out = run(generator=gen()).cpu().numpy()
    ref = z[f"{tag}_final"]
    print(f"{tag} graphs {graphs}: free-running final latents rel err {rel_err(out, ref):.3e}, PSNR {psnr(out, ref):.1f} dB")
    assert rel_err(out, ref) < 1e-2 and psnr(out, ref) > 40.0
    if seeded and "generator" not in over:          # the tapped noise (n - 1 slices, then anything) as variance_noise: the same result
        noise = torch.from_numpy(z[f"{tag}_noise"])
        out2 = run(variance_noise=torch.cat([noise, torch.full_like(noise[:1], 1e6)], 0)).cpu().numpy()
        assert np.array_equal(out, out2)
    return out


@pytest.mark.parametrize("tag", ["lcm_cfg_4", "lcm_nocfg_4", "ddim_single_5", "unipc_single_5", "lcm_wcond_4", "lcm_wcond_custom_3"])
@pytest.mark.parametrize("graphs", [False, True])
def test_lcm_loop_matches_the_reference(tag, graphs):
    z = np.load(os.path.join(GOLD, "loop_tiny_lcm.npz"))
    usd, bsd = tiny_weights()
    a = _loop_inputs()
    wcond = "wcond" in tag
    eng = _cond_engine(graphs) if wcond else make_pipeline(usd, bsd, scheduler="unipc", use_graphs=graphs)
    kw = json.loads(str(z[f"{tag}_kw"]))
    guidance_free, B = float(kw["guidance_scale"]) <= 1.0 or wcond, int(kw["batch"])
    over = dict(single_pass=True) if tag in ("ddim_single_5", "unipc_single_5") else {}      # (LCM, a time-cond UNet: the default decides)
    _check_case(eng, z, tag, a, graphs, **over)
    keys = list(eng._plans)
    assert len(keys) == 1 and (keys[0][-1] == "single") == guidance_free and keys[0][0] == B, keys
    P = eng._plans[keys[0]]
    assert P.single == guidance_free and P.ctx.shape[0] == (B if guidance_free else 2 * B) and P.unet_in.shape[0] == P.ctx.shape[0]
    assert (P.timestep_cond is not None) == wcond
    assert eng.cache_stats["plans_recorded"] == 1 and eng.cache_stats["loop_graph_captures"] == (1 if graphs else 0)


@pytest.mark.parametrize("graphs", [False, True])
def test_guidance_free_lcm_on_the_duplicated_plan_meets_the_same_bar(graphs):
    """single_pass=False: both CFG halves hold the positive prompt, effective scale 1 - what every guidance-free call ran on before."""
    z = np.load(os.path.join(GOLD, "loop_tiny_lcm.npz"))
    usd, bsd = tiny_weights()
    a = _loop_inputs()
    eng = make_pipeline(usd, bsd, scheduler="unipc", use_graphs=graphs)
    dup = _check_case(eng, z, "lcm_nocfg_4", a, graphs, single_pass=False)
    assert [k[-1] for k in eng._plans] != ["single"] and len(eng._plans) == 1 and not next(iter(eng._plans.values())).single
    one = _check_case(eng, z, "lcm_nocfg_4", a, graphs)
    assert len(eng._plans) == 2 and list(eng._plans)[-1][-1] == "single"
    print(f"single-pass vs duplicated plan: rel {rel_err(one, dup):.3e}")
    # both halves of the positive prompt given, scale <= 1: the single-pass plan takes the second half
    run, _ = _run_case(eng, z, "lcm_nocfg_4", a)
    both = eng.denoise(torch.cat([a["prompt"][:1] * 3.0, a["prompt"][1:]]), a["fg"], a["bg"], a["score"], a["dino"], num_inference_steps=4,
                       guidance_scale=1.0, latents=a["latents"], blobnet_control_guidance_end=0.5, do_classifier_free_guidance=True,
                       generator=torch.Generator().manual_seed(int(z["lcm_nocfg_4_seed"]))).cpu().numpy()
    assert np.array_equal(both, one)
    with pytest.raises(ValueError, match="single_pass"):
        eng.denoise(a["prompt"], a["fg"], a["bg"], a["score"], a["dino"], num_inference_steps=4, guidance_scale=7.5, latents=a["latents"],
                    single_pass=True)
    with pytest.raises(NotImplementedError, match="eta"):
        run(eta=0.5)


def test_another_guidance_scale_replays_the_same_time_cond_graph():
    """The guidance scale of a distilled UNet is the contents of the plan buffer `timestep_cond`: a new scale records and captures
    nothing and changes the result; no timestep_cond at all is the zero embedding's result (cond_proj has no bias)."""
    z = np.load(os.path.join(GOLD, "loop_tiny_lcm.npz"))
    from blobctrl_amd.pipeline import get_guidance_scale_embedding
    a = _loop_inputs()
    eng = _cond_engine(True)
    run, _ = _run_case(eng, z, "lcm_wcond_4", a)
    gen = lambda: torch.Generator().manual_seed(int(z["lcm_wcond_4_seed"]))
    x75 = run(generator=gen()).cpu().numpy()
    st = dict(eng.cache_stats)
    x30 = run(generator=gen(), guidance_scale=3.0, timestep_cond=get_guidance_scale_embedding(torch.tensor([2.0]), COND_DIM)).cpu().numpy()
    x75b = run(generator=gen()).cpu().numpy()
    none = run(generator=gen(), timestep_cond=None).cpu().numpy()
    zero = run(generator=gen(), timestep_cond=torch.zeros(1, COND_DIM)).cpu().numpy()
    st2 = eng.cache_stats
    assert st2["plans_recorded"] == st["plans_recorded"] == 1 and st2["loop_graph_captures"] == st["loop_graph_captures"] == 1
    assert st2["loop_graph_hits"] == st["loop_graph_hits"] + 4
    assert rel_err(x75, z["lcm_wcond_4_final"]) < 1e-2 and np.array_equal(x75, x75b) and np.array_equal(none, zero)
    assert rel_err(x30, x75) > 1e-2 and rel_err(none, x75) > 1e-2
    with pytest.raises(ValueError, match="timestep_cond"):
        run(timestep_cond=torch.zeros(2, COND_DIM))
    usd, bsd = tiny_weights()
    plain = make_pipeline(usd, bsd, scheduler="unipc", use_graphs=False)
    with pytest.raises(ValueError, match="cond_proj"):
        plain.denoise(a["prompt"], a["fg"], a["bg"], a["score"], a["dino"], num_inference_steps=2, latents=a["latents"],
                      timestep_cond=torch.zeros(1, COND_DIM))
    assert plain.cache_stats["plans_recorded"] == 0


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


def test_pipeline_call_with_the_lcm_scheduler_matches_the_reference_call(parts):
    from PIL import Image
    from blobctrl_amd.pipeline import StableDiffusionBlobNetPipeline
    from blobctrl_amd.schedulers import DDIMScheduler, LCMScheduler
    z = np.load(os.path.join(GOLD, "pipeline_call.npz"))
    zl = np.load(os.path.join(GOLD, "pipeline_call_lcm.npz"))
    kw = dict(pipeline_cases()["ddim_neg2"])
    for k in ("scheduler", "seed", "rng_seed", "num_inference_steps", "guidance_scale"):
        kw.pop(k)
    seed, rng_seed, steps = int(zl["seed"]), int(zl["rng_seed"]), int(zl["num_inference_steps"])
    pipe = StableDiffusionBlobNetPipeline(tokenizer=FakeTokenizer(), scheduler=DDIMScheduler(**SD), safety_checker=None,
                                          requires_safety_checker=False, **parts)
    common = dict(fg_image=Image.fromarray(z["fg"]), bg_image=Image.fromarray(z["bg"]), gs_score=torch.from_numpy(z["gs_score"]),
                  height=64, width=64, output_type="latent", **kw)
    src = pipe.scheduler.config
    pipe.scheduler = LCMScheduler.from_config(src)
    for tag in ("cfg", "nocfg"):
        torch.manual_seed(rng_seed)
        out = pipe(num_inference_steps=steps, guidance_scale=float(zl[f"{tag}_guidance_scale"]),
                   generator=torch.Generator().manual_seed(seed), **common)
        got, ref = out.images.cpu().numpy(), zl[f"{tag}_latents"]
        assert pipe.num_timesteps == steps and np.array_equal(pipe.scheduler.timesteps.cpu().numpy(), zl[f"{tag}_timesteps"])
        rel = rel_err(got, ref)
        print(f"__call__ lcm {tag} on {zl[f'{tag}_timesteps']}: end to end max-abs/scale {rel:.3e}, PSNR {psnr(got, ref):.1f} dB")
        assert got.shape == ref.shape and rel < 3e-2 and psnr(got, ref) > 36.0
        key = list(pipe.engine._plans)[-1]
        assert (key[-1] == "single") == (tag == "nocfg") and key[0] == 2
    # the components of a distilled LCM model: guidance 7.5 goes in as timestep_cond, no classifier-free guidance (pipe:497, 987-993)
    from blobctrl_amd.modules import UNet2DConditionModel
    usd8, ucfg8 = _cond_unet()
    cond_pipe = StableDiffusionBlobNetPipeline(tokenizer=FakeTokenizer(), scheduler=LCMScheduler.from_config(src), safety_checker=None,
                                               requires_safety_checker=False, **dict(parts, unet=UNet2DConditionModel(usd8, ucfg8)))
    torch.manual_seed(rng_seed)
    out = cond_pipe(num_inference_steps=steps, guidance_scale=float(zl["wcond_guidance_scale"]), generator=torch.Generator().manual_seed(seed),
                    **common)
    got, ref = out.images.cpu().numpy(), zl["wcond_latents"]
    assert not cond_pipe.do_classifier_free_guidance and cond_pipe.num_timesteps == steps
    print(f"__call__ lcm wcond: end to end max-abs/scale {rel_err(got, ref):.3e}, PSNR {psnr(got, ref):.1f} dB")
    assert got.shape == ref.shape and rel_err(got, ref) < 3e-2 and psnr(got, ref) > 36.0
    key = list(cond_pipe.engine._plans)[-1]
    assert key[-1] == "single" and key[0] == 2 and rel_err(zl["wcond_latents"], zl["nocfg_latents"]) > 3e-2
    # caller timesteps are taken; eta is refused as for every scheduler but DDIM
    out = pipe(timesteps=[939, 601, 320, 19], guidance_scale=1.0, generator=torch.Generator().manual_seed(seed), **common)
    assert pipe.num_timesteps == 4 and pipe.scheduler.timesteps.tolist() == [939, 601, 320, 19] and torch.isfinite(out.images).all()
    with pytest.raises(NotImplementedError, match="eta"):
        pipe(num_inference_steps=steps, eta=0.5, generator=torch.Generator().manual_seed(seed), **common)


# ------------------------------------------------------------------------------------------------------------------ caches
def test_unipc_lcm_unipc_keep_their_own_plans_and_each_matches_its_reference():
    usd, bsd = tiny_weights()
    a = _loop_inputs()
    zl = np.load(os.path.join(GOLD, "loop_tiny.npz"))
    z = np.load(os.path.join(GOLD, "loop_tiny_lcm.npz"))
    eng = make_pipeline(usd, bsd, scheduler="unipc", use_graphs=True)

    def uni():
        _use(eng, "unipc")
        return eng.denoise(a["prompt"], a["fg"], a["bg"], a["score"], a["dino"], num_inference_steps=6, guidance_scale=7.5,
                           latents=a["latents"], blobnet_control_guidance_start=0.0, blobnet_control_guidance_end=0.67).cpu().numpy()

    def lcm(tag):
        run, _ = _run_case(eng, z, tag, a)
        return run(generator=torch.Generator().manual_seed(int(z[f"{tag}_seed"]))).cpu().numpy()

    x_u = uni()
    st = dict(eng.cache_stats)
    x_l = lcm("lcm_nocfg_4")
    x_c = lcm("lcm_cfg_4")
    st1 = dict(eng.cache_stats)
    # the single-pass LCM edit and the guided LCM edit never replay UniPC's launches, nor each other's
    assert st1["plans_recorded"] == st["plans_recorded"] + 2 and st1["loop_graph_captures"] == st["loop_graph_captures"] + 2
    assert st1["plan_hits"] == st["plan_hits"] and st1["loop_graph_hits"] == st["loop_graph_hits"]
    x_u2, x_l2, x_c2 = uni(), lcm("lcm_nocfg_4"), lcm("lcm_cfg_4")
    st2 = eng.cache_stats
    assert st2["plans_recorded"] == st1["plans_recorded"] and st2["loop_graph_captures"] == st1["loop_graph_captures"]
    assert st2["plan_hits"] == st1["plan_hits"] + 3 and st2["loop_graph_hits"] == st1["loop_graph_hits"] + 3
    for got, ref, what in ((x_u, zl["unipc_6_final"], "unipc"), (x_l, z["lcm_nocfg_4_final"], "lcm single-pass"),
                           (x_c, z["lcm_cfg_4_final"], "lcm guided"), (x_u2, zl["unipc_6_final"], "unipc again")):
        print(f"{what}: rel err {rel_err(got, ref):.3e}, PSNR {psnr(got, ref):.1f} dB")
        assert rel_err(got, ref) < 1e-2 and psnr(got, ref) > 40.0, what
    assert np.array_equal(x_u, x_u2) and np.array_equal(x_l, x_l2) and np.array_equal(x_c, x_c2)


# ------------------------------------------------------------------------------------------------------------------ plan runtime
def test_c_host_replays_a_compiled_single_pass_lcm_plan_to_the_engines_latents(tmp_path):
    """tools/make_plan_fixture.py compiles the guidance-free LCM edit WITHOUT a GPU (a version-7 file: its steps end in
    bc_scheduler_step_single, `ctx` holds the positive prompt only); the unchanged tests/c/plan_edit.c loads it with bc_plan_load and
    runs it eagerly, with per-step graphs and as one whole-loop graph: each must land on what the in-process engine computed for the
    same edit (plan_edit's own bar: 1e-2 of scale)."""
    z = np.load(os.path.join(GOLD, "loop_tiny_lcm.npz"))
    tag = "lcm_nocfg_4"
    usd, bsd = tiny_weights()
    a = _loop_inputs()
    eng = make_pipeline(usd, bsd, scheduler="unipc", use_graphs=False)
    run, _ = _run_case(eng, z, tag, a)
    mine = run(generator=torch.Generator().manual_seed(int(z[f"{tag}_seed"]))).cpu().numpy()
    assert rel_err(mine, z[f"{tag}_final"]) < 1e-2 and list(eng._plans)[-1][-1] == "single"
    np.save(tmp_path / "expected.npy", mine)
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")          # the compile step must not need a GPU
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "make_plan_fixture.py"), str(tmp_path), "--lcm", tag, "--expected",
                        str(tmp_path / "expected.npy")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(tmp_path / "tiny_edit.bcplan", "rb").read()[4:8] == (7).to_bytes(4, "little")
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
