"""FreeU on MI355X: bc_freeu against a float64 restatement of the closed form on its own fp16 inputs, the UNet module shell against the
reference's `enable_freeu` forward (tests/golden/unet_tiny_freeu.npz), and the pipeline's `__call__` against the reference's own after
`pipe.enable_freeu(...)` (pipeline_call_freeu.npz).

Bars.  Kernel: the filtered skip within |err| <= 2^-10 |want| + 2^-12 max|x| of its (image, channel) map - one fp16 rounding of the
result (2^-11 relative) plus an absolute term more than 100 x the fp32 accumulation error of <= 1152 addends and far below the filter's
own effect; the scaled half of hidden bit-equal to (h.float() * b).half(), everything else bit-equal to the input; the emitted totals at
the rtol 1e-4 / atol 1e-2 of the other totals tests.  Nets: the project's HIP-versus-reference bar, max-abs / scale < 1e-2 and PSNR >
40 dB.  The single-pass and Euler FreeU edits have no reference fixture: they are held bit for bit to the eager replay of their own
plans, and to nothing else."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.common import PIPE, TINY, FakeTokenizer, g, pipeline_cases, psnr, tiny_pipeline_weights, tiny_weights  # noqa: E402
from tests.gpu_common import make_pipeline, tiny_trunk_configs  # noqa: E402
from tests.test_freeu_cpu import fourier_filter_closed  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000, steps_offset=1)
DEV = "cuda:0"
FREEU = (0.9, 0.2, 1.5, 1.6)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


# ------------------------------------------------------------------------------------------------------------------ kernel
def _check_launch(hidden, skip, params, stage):
    """One launch on (hidden, skip) [B][H][W][C] fp16 with params (s1, s2, b1, b2) against the float64 restatement; returns skip_out."""
    from blobctrl_amd import ops
    from blobctrl_amd.launch import decode_gn_tot, gn_tot_slots
    B, H, W, C_h = hidden.shape
    h0, s0 = hidden.clone(), skip.clone()
    pdev = torch.tensor(params, dtype=torch.float32, device=DEV)
    h_out, s_out, tot_h, tot_s = ops.freeu_launch(hidden, skip, pdev, stage)
    torch.cuda.synchronize()
    assert torch.equal(hidden, h0) and torch.equal(skip, s0)                           # the inputs are not modified
    s, b = float(np.float32(params[stage])), params[2 + stage]
    # hidden: the lower half of the channels scaled with one fp16 rounding, the rest copied bit for bit
    half = C_h // 2
    assert torch.equal(h_out[..., :half], (hidden[..., :half].float() * b).half()) and torch.equal(h_out[..., half:], hidden[..., half:])
    # skip: the closed form in float64 on the fp16 inputs
    x = skip.permute(0, 3, 1, 2).double().cpu()
    want = fourier_filter_closed(x, s)
    got = s_out.permute(0, 3, 1, 2).double().cpu()
    bound = 2.0 ** -10 * want.abs() + 2.0 ** -12 * x.abs().amax(dim=(2, 3), keepdim=True)
    worst = ((got - want).abs() / bound).max().item()
    print(f"freeu {tuple(hidden.shape)} | {skip.shape[-1]} stage {stage}: worst |err| / bound {worst:.3f}, filter moved the data by "
          f"{(want - x).abs().max().item():.3f}")
    assert ((got - want).abs() <= bound).all()
    assert (want - x).abs().max().item() > 8 * bound.max().item()                      # (the bound is far below the filter's effect)
    # the GroupNorm statistics totals: sums of the STORED fp16 values, per channel
    for out, tot in ((h_out, tot_h), (s_out, tot_s)):
        v = out.double().reshape(B, H * W, -1)
        sums = torch.stack([v.sum(1), (v * v).sum(1)], -1).cpu()                       # [B][C][2]
        dec = decode_gn_tot(tot)
        assert torch.allclose(dec, sums, rtol=1e-4, atol=1e-2)
        assert torch.allclose(gn_tot_slots(dec), gn_tot_slots(sums), rtol=1e-4, atol=1e-2)
    return s_out, h_out


@pytest.mark.parametrize("B,H,W,C_h,C_s", [(2, 4, 8, 64, 64), (2, 3, 6, 64, 32), (1, 1, 2, 16, 16), (2, 2, 2, 32, 64), (2, 8, 16, 1280, 1280),
                                           (2, 16, 32, 1280, 640), (1, 12, 24, 1280, 1280)])
def test_kernel_against_the_float64_closed_form(B, H, W, C_h, C_s):
    gen = torch.Generator().manual_seed(1000 * H + W + C_s)
    hidden = (torch.randn(B, H, W, C_h, generator=gen) + 0.5).half().to(DEV)
    # a DC offset per channel (a dropped DC term shows) on unit-scale data
    skip = (torch.randn(B, H, W, C_s, generator=gen) + 0.7 + 0.5 * torch.sin(torch.arange(C_s, dtype=torch.float32))).half().to(DEV)
    for stage in (0, 1):
        a, ha = _check_launch(hidden, skip, FREEU, stage)
        # the same arguments, other contents of the parameter buffer: the other answer (the parameters are read on the device)
        b, hb = _check_launch(hidden, skip, (0.5, 0.7, 1.2, 0.8), stage)
        assert not torch.equal(a, b) and not torch.equal(ha, hb)
    # the two stages read different entries
    assert not torch.equal(_check_launch(hidden, skip, FREEU, 0)[0], _check_launch(hidden, skip, FREEU, 1)[0])


def test_host_wrapper_refuses_bad_arguments():
    from blobctrl_amd import _lib, ops
    h = torch.zeros(1, 2, 2, 16, dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.BlobCtrlHipError, match="stage"):
        ops.freeu_launch(h, h.clone(), torch.ones(4, device=DEV), 2)
    with pytest.raises(_lib.BlobCtrlHipError, match="widths"):
        ops.freeu_launch(torch.zeros(1, 2, 2, 12, dtype=torch.float16, device=DEV), h, torch.ones(4, device=DEV), 0)
    oh, os_ = torch.ops.blobctrl.freeu(h + 1, h + 2, torch.tensor(FREEU, device=DEV), 0)
    assert oh.shape == h.shape and os_.shape == h.shape and torch.equal(oh[..., :8], torch.full_like(oh[..., :8], 1.5))


# ------------------------------------------------------------------------------------------------------------------ UNet module
def _residuals(unet, seed, scale, B, H, W):
    """The seeded residual tensors of a unet_tiny_freeu.npz case (tools/make_golden.py freeu_residuals): right-hand square slices."""
    down, mid, up = unet._res_shapes(H, W)
    sq = lambda s: (s[0], s[1], min(s[1], s[2]))
    mk = lambda i, s: (g(seed + i, B, *sq(s)) * scale).to(DEV)
    return dict(down_block_add_samples=[mk(i, s) for i, s in enumerate(down)], mid_block_add_sample=mk(100, mid),
                up_block_add_samples=[mk(200 + i, s) for i, s in enumerate(up)])


@pytest.mark.parametrize("geo", ["wide16", "wide12", "square16"])
def test_unet_module_matches_the_reference_with_freeu(geo):
    from blobctrl_amd.modules import UNet2DConditionModel
    z = np.load(os.path.join(GOLD, "unet_tiny_freeu.npz"))
    assert tuple(z["freeu"]) == FREEU and tuple(z["freeu_filter_only"]) == (0.9, 0.2, 1.0, 1.0)
    unet = UNet2DConditionModel(tiny_weights()[0], tiny_trunk_configs()[0])
    never = UNet2DConditionModel(tiny_weights()[0], tiny_trunk_configs()[0])
    x, ehs = torch.from_numpy(z[f"{geo}_unet_in"]).to(DEV), torch.from_numpy(z[f"{geo}_ehs"]).to(DEV)
    B, _, H, W = x.shape
    t = int(z["timestep"])
    res = lambda m: _residuals(m, int(z[f"{geo}_res_seed"]), float(z["res_scale"]), B, H, W)
    run = lambda m: m(x, t, encoder_hidden_states=ehs, return_dict=False, **res(m))[0].cpu().numpy()
    for what, params in (("eps", FREEU), ("eps_filter_only", (0.9, 0.2, 1.0, 1.0)), ("eps_off", None)):
        unet.enable_freeu(*params) if params is not None else unet.disable_freeu()
        got, ref = run(unet), z[f"{geo}_{what}"]
        print(f"FreeU UNet {geo} {what}: rel {rel_err(got, ref):.3e}, PSNR {psnr(got, ref):.1f} dB; vs eps_off {rel_err(ref, z[f'{geo}_eps_off']):.3f}")
        assert rel_err(got, ref) < 1e-2 and psnr(got, ref) > 40.0, what
    assert rel_err(z[f"{geo}_eps"], z[f"{geo}_eps_off"]) > 0.1 and rel_err(z[f"{geo}_eps_filter_only"], z[f"{geo}_eps_off"]) > 0.1
    # disable_freeu: bit-identical to a module that was never enabled, on the plan key it always had
    assert np.array_equal(got, run(never))
    assert sorted(len(k) for k in unet._plans) == [6, 7] and [len(k) for k in never._plans] == [6]
    # any zero among the four runs the plain plan
    unet.enable_freeu(0.9, 0.2, 0.0, 1.6)
    assert np.array_equal(run(unet), got) and len(unet._plans) == 2
    # other values replay the FreeU plan and give another answer
    unet.enable_freeu(0.6, 0.4, 1.2, 1.4)
    other = run(unet)
    assert len(unet._plans) == 2 and rel_err(other, z[f"{geo}_eps"]) > 1e-2


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


def test_pipeline_call_with_freeu_matches_the_reference_call(parts):
    """The reference's own `__call__` after enable_freeu, keyword for keyword, with the whole-edit graph on; then the loop from the
    reference's loop-entry tensors; other values on the same plan and graph; the eager path bit for bit."""
    from PIL import Image
    from blobctrl_amd.pipeline import StableDiffusionBlobNetPipeline
    from blobctrl_amd.schedulers import DDIMScheduler
    z = np.load(os.path.join(GOLD, "pipeline_call.npz"))
    zf = np.load(os.path.join(GOLD, "pipeline_call_freeu.npz"))
    kw = dict(pipeline_cases()["ddim_neg2"])
    for k in ("scheduler", "seed", "rng_seed", "num_inference_steps"):
        kw.pop(k)
    seed, rng_seed, steps = int(zf["seed"]), int(zf["rng_seed"]), int(zf["num_inference_steps"])
    other = tuple(float(v) for v in zf["freeu_other"])
    mk = lambda graphs: StableDiffusionBlobNetPipeline(tokenizer=FakeTokenizer(), scheduler=DDIMScheduler(**SD), safety_checker=None,
                                                       requires_safety_checker=False, use_graphs=graphs, **parts)
    pipe = mk(True)
    common = dict(fg_image=Image.fromarray(z["fg"]), bg_image=Image.fromarray(z["bg"]), gs_score=torch.from_numpy(z["gs_score"]),
                  height=64, width=64, output_type="latent", num_inference_steps=steps, **kw)

    def call(p):
        torch.manual_seed(rng_seed)
        return p(generator=torch.Generator().manual_seed(seed), **common).images.cpu().numpy()
    try:
        pipe.enable_freeu(*(float(v) for v in zf["freeu"]))
        assert parts["unet"].freeu == FREEU
        got, ref = call(pipe), zf["latents"]
        eng = pipe.engine
        assert eng.loop_graph and list(eng._plans)[-1][-1] == "freeu" and eng.cache_stats["loop_graph_captures"] == 1
        print(f"__call__ freeu: end to end max-abs/scale {rel_err(got, ref):.3e}, PSNR {psnr(got, ref):.1f} dB; "
              f"reference on vs off {rel_err(ref, zf['latents_off']):.3f}")
        assert got.shape == ref.shape and rel_err(got, ref) < 1e-2 and psnr(got, ref) > 40.0
        # the loop from the reference's own loop-entry tensors
        t = lambda k: torch.from_numpy(zf[f"entry_{k}"])
        noise = torch.randn((2, 4, 8, 8), generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
        loop = eng.denoise(torch.cat([t("negative_prompt_embeds"), t("prompt_embeds")]), t("fg_latents"), t("bg_latents"),
                           torch.from_numpy(z["gs_score"]), t("dino"), num_inference_steps=steps, guidance_scale=float(kw["guidance_scale"]),
                           latents=noise, blobnet_conditioning_scale=kw["blobnet_conditioning_scale"],
                           blobnet_control_guidance_start=kw["blobnet_control_guidance_start"],
                           blobnet_control_guidance_end=kw["blobnet_control_guidance_end"], freeu=FREEU).cpu().numpy()
        print(f"freeu loop from the reference's entry tensors: max-abs/scale {rel_err(loop, ref):.3e}, PSNR {psnr(loop, ref):.1f} dB")
        assert rel_err(loop, ref) < 1e-2 and psnr(loop, ref) > 40.0
        # other values: a plan hit, no new capture, another answer - the reference's
        st = dict(eng.cache_stats)
        pipe.enable_freeu(*other)
        got2 = call(pipe)
        st2 = eng.cache_stats
        assert st2["plans_recorded"] == st["plans_recorded"] and st2["loop_graph_captures"] == st["loop_graph_captures"]
        assert st2["plan_hits"] == st["plan_hits"] + 1 and st2["loop_graph_hits"] == st["loop_graph_hits"] + 1
        print(f"__call__ freeu, other values: max-abs/scale {rel_err(got2, zf['latents_other']):.3e}; vs the first {rel_err(got2, got):.3f}")
        assert rel_err(got2, zf["latents_other"]) < 1e-2 and psnr(got2, zf["latents_other"]) > 40.0 and rel_err(got2, got) > 0.1
        # the eager path (no graphs) agrees bit for bit
        pipe.enable_freeu(*FREEU)
        assert np.array_equal(call(pipe), got)
        eager = mk(False)
        assert np.array_equal(call(eager), got) and eager.engine.cache_stats["loop_graph_captures"] == 0
        # disable_freeu: the plain plan, the reference's FreeU-off latents
        pipe.disable_freeu()
        off = call(pipe)
        assert "freeu" not in list(pipe.engine._plans)[-1] and len(pipe.engine._plans) == 2
        assert rel_err(off, zf["latents_off"]) < 1e-2 and psnr(off, zf["latents_off"]) > 40.0
    finally:
        parts["unet"].disable_freeu()


def _loop_inputs():
    from oracle import blob_splat
    score = torch.from_numpy(blob_splat.splat_scores_from_ellipse([[40.0, 42.0], [20.0, 30.0], 25.0], 64, 64, 8, 8))
    return dict(latents=g(31, 1, 4, 8, 8), prompt=g(32, 2, 7, TINY["ctx"]), fg=g(33, 1, 4, 8, 8) * 0.18215 * 5,
                bg=g(34, 1, 4, 8, 8) * 0.18215 * 5, score=score, dino=g(35, 1, 1, TINY["feat"]))


@pytest.mark.parametrize("what", ["single_pass", "euler"])
def test_single_pass_and_euler_freeu_edits_equal_their_eager_runs(what):
    """Compositions without a reference fixture: the whole-edit graph of a FreeU plan against the eager replay of the same plan, bit for
    bit, and against the same edit with FreeU off (it must differ)."""
    from blobctrl_amd import schedulers
    usd, bsd = tiny_weights()
    a = _loop_inputs()
    outs = {}
    for graphs in (True, False):
        eng = make_pipeline(usd, bsd, scheduler="ddim", use_graphs=graphs)
        if what == "euler":
            s = schedulers.EulerDiscreteScheduler(**SD)
            eng.set_scheduler(s.kind, s.table_params())
            kw, prompt = dict(guidance_scale=5.0), a["prompt"]
        else:
            kw, prompt = dict(guidance_scale=1.0, do_classifier_free_guidance=False, single_pass=True), a["prompt"][1:]
        run = lambda **k: eng.denoise(prompt, a["fg"], a["bg"], a["score"], a["dino"], num_inference_steps=3, latents=a["latents"],
                                      blobnet_control_guidance_end=0.67, **kw, **k).cpu().numpy()
        outs[graphs] = run(freeu=FREEU)
        key = list(eng._plans)[-1]
        assert key[-1] == "freeu" and (("single" in key) == (what == "single_pass")) and (("scaled" in key) == (what == "euler"))
        off = run()
        assert np.isfinite(outs[graphs]).all() and rel_err(outs[graphs], off) > 1e-2 and len(eng._plans) == 2
        assert eng.cache_stats["loop_graph_captures"] == (2 if graphs else 0)
    assert np.array_equal(outs[True], outs[False])
