"""Perturbed-attention guidance on MI355X (tests/pag_common.py: cases, inputs, float64 references, fenced problems).

bc_attention_identity alone in NaN-fenced buffers: bit-equal to V, nothing else written.  bc_pag_scheduler_step against float64 from its
own fp32 inputs at the bar tests/test_lcm_gpu.py holds bc_scheduler_step_single to (max-abs error <= 1e-6 of max |reference|, per
buffer).  The block as the planner records a PAG layer against the reference's Transformer2DModel with the PAG processor
(tests/golden/blocks_pag.npz) at the bar of tests/test_blocks_gpu.py; the UNet module against unet_tiny_pag.npz and the pipeline's
`__call__` against pipeline_call_pag.npz at the bar of tests/test_freeu_gpu.py (max-abs / scale < 1e-2, PSNR > 40 dB); PAG with an
IP-Adapter and FreeU against the module-level composition."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import pag_common as pc  # noqa: E402
from tests.common import PIPE, TINY, FakeTokenizer, g, pipeline_cases, psnr, tiny_pipeline_weights, tiny_weights  # noqa: E402
from tests.gpu_common import make_pipeline, tiny_trunk_configs  # noqa: E402

DEV = torch.device("cuda:0")
LAYERS = ("mid_block.attentions.0.",)                                         # what pc.PAG_CALL_LAYERS ("mid") resolves to
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000, steps_offset=1)


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


# ---------------------------------------------------------------------------------------------------- bc_attention_identity
@pytest.mark.parametrize("ldo_extra", pc.IDENTITY_LDO_EXTRA)
@pytest.mark.parametrize("heads,d", pc.IDENTITY_HEADS)
@pytest.mark.parametrize("HW", pc.IDENTITY_TOKENS)
def test_attention_identity_is_a_bit_exact_transpose_copy(HW, heads, d, ldo_extra):
    """Every (B, b0) at one shape: rows [b0 HW, B HW) bit-equal to V, the rows of the images in front still the sentinel pattern, no NaN of
    V^T's pad columns anywhere in the view, every bit outside the view (the fence columns C .. ldo among them) as it was."""
    from blobctrl_amd.launch import Recorder
    for B, b0 in pc.IDENTITY_BATCHES:
        prob = pc.IdentityProblem(DEV, B, b0, HW, heads, d, ldo_extra)
        prob.assert_inside()
        prob.o.snapshot()
        rec = Recorder(DEV)
        try:
            seg = rec.begin("launch")
            rec.attention_identity(*prob.args())
            seg.run(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert dict(seg.kinds) == {"attention_identity": 1}
        finally:
            rec.close()
        what = f"attention_identity B={B} b0={b0} HW={HW} C={heads * d} ldo={prob.ldo}"
        vals, fenced = prob.o.check(what)                                   # nothing outside the view written, nothing non-finite inside
        want = prob.expected()
        got = prob.o.v.valid().cpu()
        assert fenced > 0 and torch.equal(got.view(torch.int16), want.view(torch.int16)), what
        assert torch.equal(got[: b0 * HW], prob.before[: b0 * HW]) and not torch.equal(got[b0 * HW:], prob.before[b0 * HW:]), what
    # b0 == B: nothing to do, nothing touched
    prob = pc.IdentityProblem(DEV, 2, 2, HW, heads, d, ldo_extra)
    prob.o.snapshot()
    from blobctrl_amd import _lib
    args = prob.args()
    _lib.check(_lib.load().bc_attention_identity(args[0].data_ptr(), args[1].data_ptr(), *args[2:], C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert prob.o.untouched()


# ---------------------------------------------------------------------------------------------------- bc_pag_scheduler_step
@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("form", pc.STEP_FORMS)
def test_pag_step_against_float64(form, single):
    """B = 2, h = 3, w = 5 at step 1 of 4: eps_out, latents and the three history slots against float64 from the launch's own fp32 inputs.
    The inputs can see a wrong launch (asserted from the reference alone); a step index outside [0, nsteps) leaves every buffer alone."""
    from blobctrl_amd import _lib
    lib = _lib.load()
    inp = pc.step_inputs(form, single)
    power = pc.step_power(inp, form, single)
    print(f"pag step {form} single={single}: elements that see a wrong launch {power}")
    assert min(power.values()) >= 0.5, power
    B, h, w, N = pc.STEP_B, pc.STEP_H, pc.STEP_W, pc.STEP_N
    dev = {k: v.to(DEV).contiguous() for k, v in inp.items() if torch.is_tensor(v)}
    x, hist = dev["x"].clone(), dev["hist"].clone()
    idx = torch.full((1,), inp["step"], dtype=torch.int32, device=DEV)
    eps_out = torch.zeros(B, 4, h, w, device=DEV)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    step = lambda adv: _lib.check(lib.bc_pag_scheduler_step(
        dev["tok"].data_ptr(), x.data_ptr(), dev["coef"].data_ptr(), idx.data_ptr(), hist.data_ptr(), dev["pag_table"].data_ptr(), B, h, w,
        dev["noise"].data_ptr() if form == "noise" else None, N, int(form == "third"), int(single), eps_out.data_ptr(), adv, stream()),
        "bc_pag_scheduler_step")
    step(1)
    torch.cuda.synchronize()
    e_ref, x_ref, hist_ref = pc.step_reference(inp, form, single)
    for got, ref, what in ((eps_out, e_ref, "eps_out"), (x, x_ref, "latents"), (hist, hist_ref, "hist")):
        assert torch.isfinite(got).all(), (form, single, what)
        err = (got.cpu().double() - ref.reshape(got.shape)).abs().max().item() / ref.abs().max().item()
        print(f"MARGIN pag step {form} single={single} {what}: max-abs err / max|ref| {err:.2e} (bar {pc.STEP_BAR:.0e})")
        assert err <= pc.STEP_BAR, (form, single, what, err)
    assert int(idx.item()) == inp["step"] + 1
    # no table row for this index: nothing is written, the counter still advances when asked
    before = [t.clone() for t in (x, hist, eps_out)]
    for bad in (N, -1, N + 7):
        idx.fill_(bad)
        step(1)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, (x, hist, eps_out))) and int(idx.item()) == bad + 1, bad
    idx.fill_(-3)
    step(0)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (x, hist, eps_out))) and int(idx.item()) == -3


# ---------------------------------------------------------------------------------------------------- one block with the PAG processor
@pytest.fixture(scope="module")
def zb(golden_dir):
    return np.load(os.path.join(golden_dir, "blocks_pag.npz"))


@pytest.mark.parametrize("name,form", [("pag_320", "rowchain"), ("pag_320", "unfused"), ("pag_640", "rowchain"), ("pag_1280", "gw"),
                                       ("pag_320_nocfg", "rowchain")])
def test_block_with_a_perturbed_chunk(zb, name, form, monkeypatch):
    """The reference's Transformer2DModel with the PAG processor on attn1 against the block as TrunkPlan records a PAG layer, in each form -
    asserted from the launch listing - at the bar of tests/test_blocks_gpu.py; the perturbed chunk is NOT within that bar of the cond chunk."""
    from tests.common import set_plan
    from tests.test_blocks_gpu import _check, _nchw, _run
    if form == "unfused":
        set_plan(monkeypatch, rowchain=0, gw=0)
    p = pc.PAG_BLOCK_CASES[name]
    n = p["B"] // p["chunks"]
    rec, seg, out = pc.pag_block_plan(name, DEV)
    try:
        kinds, variants = seg.kinds, [m.get("variant", "") for m in seg.meta]
        assert ("rowchain" in kinds) == (form == "rowchain") and any("gemm_wreg_kernel" in v for v in variants) == (form == "gw"), variants
        assert kinds["attention_identity"] == 1
        ident = [m for m in seg.meta if m["kind"] == "attention_identity"][0]
        assert ident["shape"] == ("attention_identity", n, p["H"] * p["W"], p["C"])
        _run(seg)
        got = _nchw(out, p["B"])
        _check(f"{name} ({form})", got, zb[name], p["sub"])
        sub = got[:, :, ::p["sub"], ::p["sub"]]
        gap = float(np.abs(sub[-n:] - sub[-2 * n:-n]).max() / (1e-2 * np.abs(zb[name]).max()))
        print(f"block {name} ({form}): perturbed vs cond chunk {gap:.1f} bars apart")
        assert gap > 1.0
    finally:
        rec.close()


# ---------------------------------------------------------------------------------------------------- the tiny UNet module
def _pag_unet_call(unet, z=None):
    x, ehs, seed = pc.pag_unet_inputs()
    B, _, H, W = x.shape
    down, mid, up = unet._res_shapes(H, W)
    sq = lambda s: (s[0], s[1], min(s[1], s[2]))
    res = dict(down_block_add_samples=[pc.pag_residual(seed + i, sq(s)).to(DEV) for i, s in enumerate(down)],
               mid_block_add_sample=pc.pag_residual(seed + 100, sq(mid)).to(DEV),
               up_block_add_samples=[pc.pag_residual(seed + 200 + i, sq(s)).to(DEV) for i, s in enumerate(up)])
    return unet(x.to(DEV), 981, encoder_hidden_states=ehs.to(DEV), return_dict=False, **res)[0].cpu().numpy()


def test_unet_module_matches_the_reference_with_pag_processors(golden_dir):
    """UNet2DConditionModel.set_pag_attn_processors + forward at batch 3 = [uncond | cond | perturbed] against the reference's forward with
    the processors PAGMixin._set_pag_attn_processor sets (tests/golden/unet_tiny_pag.npz), both layer sets, at the bar
    tests/test_freeu_gpu.py holds this UNet to; unset: bit-identical to a module that never set them, on the plan key it always had."""
    from blobctrl_amd.modules import UNet2DConditionModel
    z = np.load(os.path.join(golden_dir, "unet_tiny_pag.npz"))
    assert int(z["timestep"]) == 981
    unet = UNet2DConditionModel(pc.pag_tiny_unet_weights(), tiny_trunk_configs()[0])        # (the fixture's UNet: one weight changed, see there)
    never = UNet2DConditionModel(pc.pag_tiny_unet_weights(), tiny_trunk_configs()[0])
    off = _pag_unet_call(never)
    assert rel_err(off, z["eps_off"]) < 1e-2 and psnr(off, z["eps_off"]) > 40.0 and [len(k) for k in never._plans] == [6]
    for case, layers in pc.PAG_UNET_LAYERS.items():
        unet.set_pag_attn_processors(layers, True)
        got, ref = _pag_unet_call(unet), z[f"eps_{case}"]
        print(f"PAG UNet {case}: rel {rel_err(got, ref):.3e}, PSNR {psnr(got, ref):.1f} dB; reference on vs off {rel_err(ref, z['eps_off']):.3f}")
        assert rel_err(got, ref) < 1e-2 and psnr(got, ref) > 40.0, case
        # what PAG changed: the engine's own on - off against the reference's, at the same bar - a perturbation that is missing, or sits in
        # another layer, leaves it by the fixture's separation, at least 10 bars
        moved = np.abs((got - off) - (ref - z["eps_off"])).max() / np.abs(ref).max()
        sep = rel_err(ref, z["eps_off"]) / 1e-2
        print(f"PAG UNet {case}: on - off against the reference's {moved:.3e} of scale; the reference's on vs off {sep:.1f} bars")
        assert moved < 1e-2 and sep >= 10.0 and rel_err(got[:2], off[:2]) < 1e-2
        key = list(unet._plans)[-1]
        assert key[-1][:2] == ("pag", 3) and len(key[-1]) == 2 + len(json.loads(str(z[f"names_{case}"])))
    with pytest.raises(ValueError, match="Cannot find PAG layer"):
        unet.set_pag_attn_processors("no_such_layer")
    unet.unset_pag_attn_processors()
    assert np.array_equal(_pag_unet_call(unet), off) and sorted(len(k) for k in unet._plans) == [6, 7, 7]


# ---------------------------------------------------------------------------------------------------- __call__
@pytest.fixture(scope="module")
def parts():
    from blobctrl_amd.clip_text import CLIPTextModel
    from blobctrl_amd.dinov2 import Dinov2Model
    from blobctrl_amd.modules import BlobNetModel, UNet2DConditionModel
    from blobctrl_amd.vae import AutoencoderKL
    usd, bsd = pc.pag_tiny_unet_weights(), tiny_weights()[1]                   # (the fixture's UNet: one weight changed, see there)
    ucfg, bcfg = tiny_trunk_configs()
    vsd, csd, dsd = tiny_pipeline_weights()
    return dict(unet=UNet2DConditionModel(usd, ucfg), blobnet=BlobNetModel(bsd, bcfg),
                vae=AutoencoderKL(vsd, norm_num_groups=PIPE["vae_groups"]),
                text_encoder=CLIPTextModel(csd, num_heads=PIPE["clip"]["heads"]),
                dinov2=Dinov2Model(dsd, num_heads=PIPE["dino"]["heads"], patch_size=PIPE["dino"]["patch"]))


def _caller(parts, golden_dir, graphs=True):
    """(pipeline, call(case keywords) -> latents) on the inputs of pipeline_call_pag.npz."""
    from PIL import Image
    from blobctrl_amd.pipeline import StableDiffusionBlobNetPipeline
    from blobctrl_amd.schedulers import DDIMScheduler
    z = np.load(os.path.join(golden_dir, "pipeline_call.npz"))
    zp = np.load(os.path.join(golden_dir, "pipeline_call_pag.npz"))
    kw = dict(pipeline_cases()["ddim_neg2"])
    for k in ("scheduler", "seed", "rng_seed", "num_inference_steps"):
        kw.pop(k)
    seed, rng_seed, steps = int(zp["seed"]), int(zp["rng_seed"]), int(zp["num_inference_steps"])
    assert (seed, rng_seed) == (pc.PAG_CALL_SEEDS["seed"], pc.PAG_CALL_SEEDS["rng_seed"])
    pipe = StableDiffusionBlobNetPipeline(tokenizer=FakeTokenizer(), scheduler=DDIMScheduler(**SD), safety_checker=None,
                                          requires_safety_checker=False, pag_applied_layers=pc.PAG_CALL_LAYERS, use_graphs=graphs, **parts)
    common = dict(fg_image=Image.fromarray(z["fg"]), bg_image=Image.fromarray(z["bg"]), gs_score=torch.from_numpy(z["gs_score"]),
                  height=64, width=64, output_type="latent", num_inference_steps=steps)

    def call(**extra):
        torch.manual_seed(rng_seed)
        return pipe(generator=torch.Generator().manual_seed(seed), **{**common, **kw, **extra}).images.cpu().numpy()
    return pipe, call, zp


def test_pipeline_call_with_pag_matches_the_reference_call(parts, golden_dir):
    """Every case of tests/golden/pipeline_call_pag.npz - the reference's own `__call__` around a UNet that computes the PAG batch - keyword
    for keyword with the whole-edit graph on, at 1e-2 of the latents' scale.  pag_scale = 0 is the call without the keywords, bit for bit,
    and records nothing; another pag_scale or pag_adaptive_scale replays the plan and the graph of the first; a PAG-less call after the PAG
    calls returns the bits it returned before."""
    from blobctrl_amd.schedulers import DDIMScheduler, EulerDiscreteScheduler
    pipe, call, zp = _caller(parts, golden_dir)
    eng = pipe.engine
    plain = call()
    st0 = dict(eng.cache_stats)
    assert rel_err(plain, zp["off_latents"]) < 1e-2 and psnr(plain, zp["off_latents"]) > 40.0
    zero = call(pag_scale=0.0, pag_adaptive_scale=0.3)
    assert np.array_equal(zero, plain) and eng.cache_stats["plans_recorded"] == st0["plans_recorded"] and len(eng._plans) == 1
    assert not pipe.do_perturbed_attention_guidance and pipe.pag_adaptive_scale == 0.3
    figures = {}
    for case in ("pag", "adaptive", "half"):
        got, ref = call(**pc.PAG_CALL_CASES[case]), zp[f"{case}_latents"]
        figures[case] = (rel_err(got, ref), psnr(got, ref), rel_err(ref, zp["off_latents"]))
        print(f"__call__ PAG {case}: end to end max-abs/scale {figures[case][0]:.3e}, PSNR {figures[case][1]:.1f} dB; reference vs off {figures[case][2]:.3f}")
        if case == "pag":
            st1 = dict(eng.cache_stats)
            key = list(eng._plans)[-1]
            assert key[-1] == ("pag",) + LAYERS and len(eng._plans) == 2 and st1["plans_recorded"] == st0["plans_recorded"] + 1
            assert pipe.do_perturbed_attention_guidance and pipe.pag_scale == 3.0 and not pipe.do_pag_adaptive_scaling
    st2 = eng.cache_stats
    assert st2["plans_recorded"] == st1["plans_recorded"] and st2["loop_graph_captures"] == st1["loop_graph_captures"] and len(eng._plans) == 2
    assert st2["loop_graph_hits"] == st1["loop_graph_hits"] + 2 and pipe.pag_scale == 1.5
    for case, (rel, db, _) in figures.items():
        assert rel < 1e-2 and db > 40.0, (case, rel, db)
    # a PAG-less call after the PAG calls: the plan and the bits of before
    assert np.array_equal(call(), plain) and len(eng._plans) == 2
    # guidance-free: PAG is the only guidance, on [cond | perturbed]
    for case in ("nocfg_off", "nocfg"):
        got, ref = call(**pc.PAG_CALL_CASES[case]), zp[f"{case}_latents"]
        print(f"__call__ PAG {case}: end to end max-abs/scale {rel_err(got, ref):.3e}, PSNR {psnr(got, ref):.1f} dB")
        assert rel_err(got, ref) < 1e-2 and psnr(got, ref) > 40.0, case
    key = list(eng._plans)[-1]
    assert key[-2:] == ("single", ("pag",) + LAYERS) and eng._plans[key].ctx.shape[0] == 2 * plain.shape[0]
    # a table that scales the model input
    pipe.scheduler = EulerDiscreteScheduler.from_config(DDIMScheduler(**SD).config)
    for case in ("euler_off", "euler"):
        got, ref = call(**pc.PAG_CALL_CASES[case]), zp[f"{case}_latents"]
        assert np.array_equal(pipe.scheduler.timesteps.cpu().numpy(), zp[f"{case}_timesteps"])
        print(f"__call__ PAG {case}: end to end max-abs/scale {rel_err(got, ref):.3e}, PSNR {psnr(got, ref):.1f} dB")
        assert rel_err(got, ref) < 1e-2 and psnr(got, ref) > 40.0, case
    assert "scaled" in list(eng._plans)[-1] and list(eng._plans)[-1][-1][0] == "pag"


def test_pag_graph_and_eager_paths_agree_and_layers_can_change(parts, golden_dir):
    """The eager replay of a PAG plan gives the graph's bits; other layers are another plan and another answer; a layer id that matches
    nothing is the reference's ValueError; lists for the scales are refused."""
    pipe, call, zp = _caller(parts, golden_dir)
    got = call(pag_scale=3.0)
    assert rel_err(got, zp["pag_latents"]) < 1e-2 and pipe.engine.cache_stats["loop_graph_captures"] == 1
    eager, call_eager, _ = _caller(parts, golden_dir, graphs=False)
    assert np.array_equal(call_eager(pag_scale=3.0), got) and eager.engine.cache_stats["loop_graph_captures"] == 0
    assert eager.pag_applied_layers == ["mid"]
    pipe.set_pag_applied_layers(["down_blocks.1", "up_blocks.(1|2)"])
    other = call(pag_scale=3.0)
    key = list(pipe.engine._plans)[-1]
    assert len(key[-1]) == 1 + 2 + 6 and np.isfinite(other).all() and rel_err(other, zp["off_latents"]) > 1e-2
    pipe.set_pag_applied_layers("no_such_layer")
    with pytest.raises(ValueError, match="Cannot find PAG layer"):
        call(pag_scale=3.0)
    assert np.isfinite(call()).all()                                     # (inactive PAG never looks at the layers)
    pipe.set_pag_applied_layers("mid")
    assert list(pipe.engine._plans)[-1][-1] != ("pag", "mid_block.attentions.0.")
    assert np.array_equal(call(pag_scale=3.0), got) and list(pipe.engine._plans)[-1][-1] == ("pag", "mid_block.attentions.0.")
    with pytest.raises(NotImplementedError, match="one value per call"):
        call(pag_scale=[3.0, 1.0])


# ---------------------------------------------------------------------------------------------------- PAG + IP-Adapter + FreeU
def test_pag_with_an_ip_adapter_and_freeu_equals_the_module_composition():
    """One DDIM step of the engine with PAG on twelve layers, an IP-Adapter loaded and FreeU on, against the composition of the module shells: the
    BlobNet module's residuals, the UNet module (the same adapter, FreeU values and PAG processors) at batch 3 = [uncond | cond | perturbed],
    then the guidance and the step of tests/pag_common.py in float64 on the host.  Both sides run the same kernels on the same numbers
    up to the assembly of their inputs: the bar is 1e-2 of the latents' scale, and PAG, FreeU and the adapter each move the result by more."""
    from blobctrl_amd import pag, schedulers
    from blobctrl_amd.modules import BlobNetModel, UNet2DConditionModel
    from blobctrl_amd.weights import ip_adapter_on_device
    from oracle import blob_splat, pipeline as o_pipe
    from tests import ip_adapter_common as ip
    from tests.test_freeu_gpu import FREEU
    usd, bsd = tiny_weights()
    ucfg, bcfg = tiny_trunk_configs()
    unet, blob = UNet2DConditionModel(usd, ucfg), BlobNetModel(bsd, bcfg)
    unet.load_ip_adapter_weights([ip.tiny_ip_adapter(0)])
    unet.set_ip_adapter_scale(0.8)
    score = torch.from_numpy(blob_splat.splat_scores_from_ellipse([[40.0, 42.0], [20.0, 30.0], 25.0], 64, 64, 8, 8)).float()
    lat, prompt = g(31, 1, 4, 8, 8), g(32, 2, 7, TINY["ctx"])
    fg, bg, dino = g(33, 1, 4, 8, 8) * 0.18215 * 5, g(34, 1, 4, 8, 8) * 0.18215 * 5, g(35, 1, 1, TINY["feat"])
    embeds = torch.cat([torch.zeros(1, 1, ip.IP_EMBED_DIM), 3.0 * g(36, 1, 1, ip.IP_EMBED_DIM)], 0)
    gs, s_pag = 5.0, 3.0
    mid = pag.resolve_layers(ucfg, ["down_blocks.1", "mid", "up"])
    eng = make_pipeline(usd, bsd, scheduler="ddim")
    eng.set_ip_adapters(unet.__dict__["ip_adapters"])
    run = lambda **kw: eng.denoise(prompt, fg, bg, score, dino, num_inference_steps=1, guidance_scale=gs, latents=lat,
                                   ip_adapter_image_embeds=[embeds], **kw).cpu().double()
    got = run(freeu=FREEU, pag_scale=s_pag, pag_applied_layers=mid)
    key = list(eng._plans)[-1]
    assert "freeu" in key and key[-1] == ("pag",) + mid and any(isinstance(k, tuple) and k[:1] == ("ip",) for k in key)
    # ---- the composition
    tab = schedulers.DDIMTable().set_timesteps(1)
    t = int(tab.timesteps[0])
    bg_s, fg_s = score.unbind(dim=1)
    feats = torch.einsum("nmhw,nmc->nchw", fg_s.unsqueeze(1), dino).contiguous()
    down, midr, up = blob(o_pipe.construct_input(lat, fg_s.unsqueeze(1), fg, feats).to(DEV), t, conditioning_scale=1.0, return_dict=False)
    sq = lambda r: r[..., -r.shape[-2]:].repeat(3, 1, 1, 1)
    unet.enable_freeu(*FREEU)
    unet.set_pag_attn_processors(["down_blocks.1", "mid", "up"], True)
    x3 = o_pipe.construct_input(lat, bg_s.unsqueeze(1), bg).repeat(3, 1, 1, 1).to(DEV)
    dup = lambda v: torch.cat([v, v[-1:]], 0).to(DEV)
    eps = unet(x3, t, encoder_hidden_states=dup(prompt), added_cond_kwargs={"image_embeds": [dup(embeds)]}, return_dict=False,
               down_block_add_samples=[sq(r) for r in down], mid_block_add_sample=sq(midr), up_block_add_samples=[sq(r) for r in up])[0]
    eps = eps[..., eps.shape[-1] // 2:].cpu().double()
    e = pc.pag_guidance(eps, 1, gs, s_pag, False)
    want, _ = pc.host_step(tab.coef[0], e, lat * tab.init_noise_sigma, torch.zeros(3, lat.numel()), None, False)
    err = rel_err(got.numpy(), want.numpy())
    moved = {k: rel_err(run(**kw).numpy(), want.numpy()) for k, kw in (("no pag", dict(freeu=FREEU)), ("no freeu", dict(pag_scale=s_pag, pag_applied_layers=mid)))}
    eng.ip_adapters[0]["scales"].zero_()
    moved["adapter scale 0"] = rel_err(run(freeu=FREEU, pag_scale=s_pag, pag_applied_layers=mid).numpy(), want.numpy())
    print(f"PAG + IP-Adapter + FreeU, one step: max-abs/scale vs the module composition {err:.3e}; without each part {moved}")
    assert err < 1e-2 and min(moved.values()) > 1e-2, (err, moved)
