"""Masked edits on the GPU: bc_blend_scheduler_step alone against float64 and, with a binary mask, bit for bit against the entry point it
replaces; bc_blend_mask in fenced buffers; the pipeline call against tests/golden/pipeline_call_blend.npz eagerly and with the whole-edit
graph; the blend composed with PAG, FreeU and an IP-Adapter; the image and mask forms of the pipeline call; edit_region_masks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import blend_common as bc  # noqa: E402
from tests.common import PIPE, TINY, FakeTokenizer, g, pipeline_cases, psnr, tiny_pipeline_weights, tiny_weights  # noqa: E402
from tests.gpu_common import make_pipeline, tiny_trunk_configs  # noqa: E402

DEV = torch.device("cuda:0")
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000, steps_offset=1)


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


# ---------------------------------------------------------------------------------------------------- bc_blend_scheduler_step
class _Step:
    """One step launch on device copies of tests/blend_common.py step_inputs, through the entry point `PlanSpec.step_call()` names -
    with `blend` the new one, without it the one the plan would otherwise end in - on the same inputs."""

    def __init__(self, inp, form, single):
        from blobctrl_amd import _lib
        self.lib, self.inp, self.form, self.single = _lib.load(), inp, form, single
        self.B, self.h, self.w = inp["shape"]
        self.dev = {k: v.to(DEV).contiguous() for k, v in inp.items() if torch.is_tensor(v)}
        self.reset()

    def reset(self):
        self.x, self.hist = self.dev["x"].clone(), self.dev["hist"].clone()
        self.eps_out = torch.zeros(self.B, 4, self.h, self.w, device=DEV)
        self.idx = torch.full((1,), self.inp["step"], dtype=torch.int32, device=DEV)

    def buffers(self):
        return self.x, self.hist, self.eps_out

    def launch(self, blend, advance=1):
        from blobctrl_amd import _lib
        from blobctrl_amd.edit_plan import PlanSpec
        d = self.dev
        spec = PlanSpec(self.B, self.h, self.w, 7, 16, bc.STEP_N, stochastic=self.form == "noise", third_order=self.form == "third",
                        single=self.single, pag=("x",) if "pag_table" in d else (), blend=blend)
        name, head, tail = spec.step_call()
        assert (name == "bc_blend_scheduler_step") == blend
        held = dict(pag_table=d.get("pag_table"), blend_image=d["image"], blend_noise=d["bnoise"], blend_mask=d["mask"],
                    blend_table=d["blend_table"], variance_noise=d.get("noise"))
        ptr = lambda a: (None if held[a] is None else held[a].data_ptr()) if isinstance(a, str) else a
        _lib.check(getattr(self.lib, name)(d["tok"].data_ptr(), self.x.data_ptr(), d["coef"].data_ptr(), self.idx.data_ptr(), self.hist.data_ptr(),
                                           *[ptr(a) for a in head], self.B, self.h, self.w, *[ptr(a) for a in tail], self.eps_out.data_ptr(),
                                           advance, C.c_void_p(torch.cuda.current_stream().cuda_stream)), name)
        torch.cuda.synchronize()
        return name


@pytest.mark.parametrize("pag", [False, True])
@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("form", bc.STEP_FORMS)
@pytest.mark.parametrize("shape", bc.STEP_SHAPES)
def test_blend_step_against_float64(shape, form, single, pag):
    """Step 1 of 4 with soft masks that differ per image: eps_out, latents and the three history slots against float64 from the launch's
    own fp32 inputs, at STEP_BAR per buffer."""
    inp = bc.step_inputs(shape, form, single, pag)
    assert min(bc.step_power(inp, form, single).values()) > 0.5
    s = _Step(inp, form, single)
    s.launch(blend=True)
    e_ref, x_ref, hist_ref = bc.step_reference(inp, form, single)
    for got, ref, what in ((s.eps_out, e_ref, "eps_out"), (s.x, x_ref, "latents"), (s.hist, hist_ref, "hist")):
        assert torch.isfinite(got).all(), what
        err = (got.cpu().double() - ref.reshape(got.shape)).abs().max().item() / ref.abs().max().item()
        print(f"MARGIN blend step {shape} {form} single={single} pag={pag} {what}: max-abs err / max|ref| {err:.2e} (bar {bc.STEP_BAR:.0e})")
        assert err <= bc.STEP_BAR, (what, err)
    assert int(s.idx.item()) == inp["step"] + 1


@pytest.mark.parametrize("pag", [False, True])
@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("form", bc.STEP_FORMS)
@pytest.mark.parametrize("shape", bc.STEP_SHAPES)
def test_blend_step_is_exact_with_a_binary_mask(shape, form, single, pag):
    """m == 1: the bits of the entry point the plan would otherwise end in; m == 0: the bits of a * image + s * bnoise in fp32; hist and
    eps_out: the bits of the launch without the blend; a step index of -1 or nsteps changes no buffer."""
    inp = bc.step_inputs(shape, form, single, pag, binary=True)
    s = _Step(inp, form, single)
    other = s.launch(blend=False)
    plain = [t.clone() for t in s.buffers()]
    s.reset()
    s.launch(blend=True)
    x, hist, eps_out = s.buffers()
    m = s.dev["mask"][:, None].expand(-1, 4, -1, -1)
    assert 0 < int((m == 1).sum()) < m.numel() and other != "bc_blend_scheduler_step"
    a, sg = s.dev["blend_table"][inp["step"]]
    kept = a * s.dev["image"] + sg * s.dev["bnoise"]                          # fp32, one rounding per operation
    assert torch.equal(x[m == 1], plain[0][m == 1]), other
    assert torch.equal(x[m == 0], kept[m == 0])
    assert torch.equal(hist, plain[1]) and torch.equal(eps_out, plain[2])
    before = [t.clone() for t in s.buffers()]
    for bad in (-1, bc.STEP_N):
        s.idx.fill_(bad)
        s.launch(blend=True)
        assert all(torch.equal(p, q) for p, q in zip(before, s.buffers())) and int(s.idx.item()) == bad + 1, bad


# ---------------------------------------------------------------------------------------------------- bc_blend_mask
@pytest.mark.parametrize("n,H,W", [(2, 16, 24), (1, 64, 8)])
def test_blend_mask_is_the_top_left_pixel_binarised_and_writes_nothing_else(n, H, W):
    from blobctrl_amd import _lib
    lib = _lib.load()
    gen = torch.Generator().manual_seed(5600 + H)
    mask = torch.randint(0, 256, (n, H, W), generator=gen, dtype=torch.uint8)
    mask[:, ::8, ::8] = torch.tensor([127, 128, 0, 255, 126, 129], dtype=torch.uint8).repeat(n * (H // 8) * (W // 8) // 6 + 1)[: n * (H // 8) * (W // 8)].reshape(n, H // 8, W // 8)
    cells, pad = n * (H // 8) * (W // 8), 64
    buf = torch.full((pad + cells + pad,), float("nan"), device=DEV)           # NaN fences in front of and behind the output view
    md = mask.to(DEV)
    _lib.check(lib.bc_blend_mask(md.data_ptr(), buf[pad:].data_ptr(), n, H, W, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "bc_blend_mask")
    torch.cuda.synchronize()
    out = buf.cpu()
    assert torch.isnan(out[:pad]).all() and torch.isnan(out[pad + cells:]).all()
    want = (mask[:, ::8, ::8] >= 128).float()
    assert torch.equal(out[pad:pad + cells].reshape(n, H // 8, W // 8), want) and 0 < want.sum() < cells
    assert torch.equal(md.cpu(), mask)


# ---------------------------------------------------------------------------------------------------- __call__
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


@pytest.fixture(scope="module")
def zc(golden_dir):
    return np.load(os.path.join(golden_dir, "pipeline_call_blend.npz"))


def _mask_u8(grid=bc.BLEND_MASK, seed=5700):
    """A 64 x 64 uint8 mask whose 8 x 8 cells hold `grid` * 255 in their top-left pixel and anything elsewhere."""
    m = torch.randint(0, 256, (64, 64), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8).numpy()
    m[::8, ::8] = (grid * 255).astype(np.uint8)
    return m


def _caller(parts, golden_dir, case, graphs=True):
    """(pipeline, call(**extra) -> latents) on the inputs of pipeline_call_blend.npz for one of its cases."""
    from PIL import Image
    from blobctrl_amd import schedulers
    from blobctrl_amd.pipeline import StableDiffusionBlobNetPipeline
    z = np.load(os.path.join(golden_dir, "pipeline_call.npz"))
    extra = bc.BLEND_CASES[case]
    kw = dict(pipeline_cases()["ddim_neg2"])
    for k in ("scheduler", "seed", "rng_seed"):
        kw.pop(k)
    kw["num_inference_steps"] = bc.BLEND_STEPS
    kw.update({k: v for k, v in extra.items() if k != "scheduler"})
    pipe = StableDiffusionBlobNetPipeline(tokenizer=FakeTokenizer(), scheduler=bc.make_scheduler(schedulers, extra["scheduler"], SD),
                                          safety_checker=None, requires_safety_checker=False, use_graphs=graphs, **parts)
    batch = len(kw["prompt"]) * kw.get("num_images_per_prompt", 1)
    lat, image, _ = bc.blend_inputs(batch)
    common = dict(fg_image=Image.fromarray(z["fg"]), bg_image=Image.fromarray(z["bg"]), gs_score=torch.from_numpy(z["gs_score"]),
                  height=64, width=64, output_type="latent", latents=lat)

    def call(**more):
        torch.manual_seed(bc.BLEND_SEEDS["rng_seed"])
        return pipe(generator=torch.Generator().manual_seed(bc.BLEND_SEEDS["seed"]), **{**common, **kw, **more}).images.cpu().numpy()
    return pipe, call, image


@pytest.mark.parametrize("case", list(bc.BLEND_CASES))
def test_pipeline_call_with_a_mask_matches_the_reference_call(parts, golden_dir, zc, case):
    """A case of pipeline_call_blend.npz with and without the blend, with the whole-edit graph on and eagerly, at 1e-2 of the latents' scale
    and 40 dB; outside the mask the final latents are the image latents bit for bit; a second call with another mask and image replays the
    same plan with no new graph capture."""
    from PIL import Image
    pipe, call, image = _caller(parts, golden_dir, case)
    eng = pipe.engine
    mask_pil = Image.fromarray(_mask_u8())
    plain = call()
    assert "blend" not in list(eng._plans)[-1]
    got = call(image=image, mask_image=mask_pil)
    st1 = dict(eng.cache_stats)
    assert list(eng._plans)[-1][-1] == "blend" and len(eng._plans) == 2
    for what, a, ref in (("plain", plain, zc[f"{case}_plain_latents"]), ("blend", got, zc[f"{case}_blend_latents"])):
        print(f"__call__ blend {case} {what}: max-abs/scale {rel_err(a, ref):.3e}, PSNR {psnr(a, ref):.1f} dB")
        assert rel_err(a, ref) < bc.CALL_BAR and psnr(a, ref) > 40.0, (case, what)
    keep = np.broadcast_to(bc.BLEND_MASK[None, None] == 0, got.shape)
    assert np.array_equal(got[keep], np.broadcast_to(image.numpy(), got.shape)[keep])
    # another mask and another image: the same plan, the same graph
    other_mask, other_image = np.ascontiguousarray(bc.BLEND_MASK[::-1]), image.flip(0) * 0.5
    again = call(image=other_image, mask_image=Image.fromarray(_mask_u8(other_mask, 5701)))
    st2 = eng.cache_stats
    assert st2["plans_recorded"] == st1["plans_recorded"] and st2["loop_graph_captures"] == st1["loop_graph_captures"]
    assert st2["loop_graph_hits"] == st1["loop_graph_hits"] + 1 and len(eng._plans) == 2
    keep2 = np.broadcast_to(other_mask[None, None] == 0, again.shape)
    assert np.array_equal(again[keep2], np.broadcast_to(other_image.numpy(), again.shape)[keep2]) and rel_err(again, got) > bc.CALL_BAR
    # eagerly: the same launches without a graph
    eager, call_eager, _ = _caller(parts, golden_dir, case, graphs=False)
    got_eager = call_eager(image=image, mask_image=mask_pil)
    assert eager.engine.cache_stats["loop_graph_captures"] == 0
    assert rel_err(got_eager, zc[f"{case}_blend_latents"]) < bc.CALL_BAR and psnr(got_eager, zc[f"{case}_blend_latents"]) > 40.0
    assert np.array_equal(got_eager[keep], np.broadcast_to(image.numpy(), got.shape)[keep])
    # the call without the arguments after the blend calls: the bits of before
    assert np.array_equal(call(), plain)


def test_image_and_mask_forms_agree(parts, golden_dir):
    """`mask_image` as a uint8 device tensor gives the bits of the same mask as a PIL image (and as numpy); `image` as a PIL image agrees
    with passing its `encode_latents`, which is drawn third from the global generator, behind fg and bg."""
    from PIL import Image
    pipe, call, image = _caller(parts, golden_dir, "ddim")
    m8 = _mask_u8()
    by_pil = call(image=image, mask_image=Image.fromarray(m8))
    by_dev = call(image=image, mask_image=torch.from_numpy(m8).to(DEV))
    by_dev3 = call(image=image, mask_image=torch.from_numpy(np.stack([m8, m8])).to(DEV))
    assert np.array_equal(by_dev, by_pil) and np.array_equal(by_dev3, by_pil) and np.array_equal(call(image=image, mask_image=m8), by_pil)
    z = np.load(os.path.join(golden_dir, "pipeline_call.npz"))
    pil = Image.fromarray(z["bg"][::-1].copy())
    got = call(image=pil, mask_image=Image.fromarray(m8))
    torch.manual_seed(bc.BLEND_SEEDS["rng_seed"])
    for im in (Image.fromarray(z["fg"]), Image.fromarray(z["bg"])):
        pipe.encode_latents(im, height=64, width=64)
    lat = pipe.encode_latents(pil, height=64, width=64)
    want = call(image=lat, mask_image=Image.fromarray(m8))
    err = rel_err(got, want)
    print(f"image= as PIL vs its encode_latents: max-abs/scale {err:.3e}")
    assert err < bc.CALL_BAR and rel_err(got, by_pil) > bc.CALL_BAR
    by_u8 = call(image=torch.from_numpy(z["bg"][::-1].copy()).to(DEV), mask_image=Image.fromarray(m8))
    assert rel_err(by_u8, want) < bc.CALL_BAR
    with pytest.raises(ValueError, match="go together"):
        call(image=image)


# ---------------------------------------------------------------------------------------------------- composition
def test_blend_with_pag_freeu_and_an_ip_adapter_equals_the_callback_blend():
    """Three DDIM steps of the engine with PAG, FreeU and an IP-Adapter: the fused blend against the same call without the blend arguments
    and the blend applied from callback_on_step_end in torch, at 1e-2 of the latents' scale; the blend moves the result by more."""
    from blobctrl_amd import pag
    from blobctrl_amd.modules import UNet2DConditionModel
    from oracle import blob_splat
    from tests import ip_adapter_common as ip
    from tests.test_freeu_gpu import FREEU
    usd, bsd = tiny_weights()
    ucfg, _ = tiny_trunk_configs()
    unet = UNet2DConditionModel(usd, ucfg)
    unet.load_ip_adapter_weights([ip.tiny_ip_adapter(0)])
    unet.set_ip_adapter_scale(0.8)
    score = torch.from_numpy(blob_splat.splat_scores_from_ellipse([[40.0, 42.0], [20.0, 30.0], 25.0], 64, 64, 8, 8)).float()
    lat, prompt = g(31, 1, 4, 8, 8), g(32, 2, 7, TINY["ctx"])
    fg, bg, dino = g(33, 1, 4, 8, 8) * 0.18215 * 5, g(34, 1, 4, 8, 8) * 0.18215 * 5, g(35, 1, 1, TINY["feat"])
    embeds = torch.cat([torch.zeros(1, 1, ip.IP_EMBED_DIM), 3.0 * g(36, 1, 1, ip.IP_EMBED_DIM)], 0)
    image = g(37, 1, 4, 8, 8) * 0.18215 * 5
    mask = torch.from_numpy(bc.BLEND_MASK)[None, None] * 0.75 + 0.125 * torch.from_numpy(bc.BLEND_MASK.T)[None, None]      # soft values too
    layers = pag.resolve_layers(ucfg, ["mid", "up_blocks.1"])
    eng = make_pipeline(usd, bsd, scheduler="ddim")
    eng.set_ip_adapters(unet.__dict__["ip_adapters"])
    n = 3
    run = lambda **kw: eng.denoise(prompt, fg, bg, score, dino, num_inference_steps=n, guidance_scale=5.0, latents=lat,
                                   ip_adapter_image_embeds=[embeds], freeu=FREEU, pag_scale=3.0, pag_applied_layers=layers, **kw).cpu()
    fused = run(blend_image_latents=image, blend_mask=mask)
    key = list(eng._plans)[-1]
    assert key[-1] == "blend" and key[-2] == ("pag",) + layers and "freeu" in key
    rows = eng._scheduler_table(n).blend_rows()
    seen = []

    def cb(_eng, i, t, kw):
        x = kw["latents"]
        m = mask.to(x.device)
        p = rows[i, 0].item() * image.to(x.device) + rows[i, 1].item() * lat.to(x.device)
        seen.append(i)
        return {"latents": (1 - m) * p + m * x}
    unfused = run(callback_on_step_end=cb)
    plain = run()
    err, moved = rel_err(fused.numpy(), unfused.numpy()), rel_err(plain.numpy(), unfused.numpy())
    print(f"blend + PAG + FreeU + IP-Adapter: fused vs callback blend max-abs/scale {err:.3e}; without the blend {moved:.3e}")
    assert seen == [0, 1, 2] and err < bc.CALL_BAR and moved > bc.CALL_BAR
    # a callback of a blend call sees blended latents: outside a binary mask they are the noised image
    hard = torch.from_numpy(bc.BLEND_MASK)[None]
    got = []
    run(blend_image_latents=image, blend_mask=hard, callback_on_step_end=lambda e_, i, t, kw: got.append(kw["latents"].cpu().clone()) or {})
    keep = (hard == 0)[:, None].expand(1, 4, 8, 8)
    for i in range(n):
        assert torch.equal(got[i][keep], (rows[i, 0] * image + rows[i, 1] * lat)[keep]), i


# ---------------------------------------------------------------------------------------------------- edit_region_masks
def test_edit_region_masks_are_the_union_of_the_ellipse_covers():
    from blobctrl_amd import edit_inputs
    H, W = 72, 104
    a, b, c = ((30.0, 28.0), (24.0, 14.0), 20.0), ((70.0, 40.0), (30.0, 18.0), -35.0), ((52.0, 36.0), (40.0, 30.0), 5.0)
    ops, starts, targets = ["move", "resize", "remove"], [a, b, c], [b, ((70.0, 40.0), (44.0, 26.0), -35.0), None]
    got = edit_inputs.edit_region_masks(ops, starts, targets, H, W, DEV)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, H, W) and got.is_cuda
    cover = lambda e: edit_inputs.ellipse_masks([e], H, W, DEV)[0].cpu().numpy()
    for i, (s, t) in enumerate(zip(starts, targets)):
        want = cover(s) | (cover(t) if t is not None else cover(s))
        assert np.array_equal(got[i].cpu().numpy(), want) and set(np.unique(want)) == {0, 255}, ops[i]
    assert (got[0].cpu().numpy() != cover(a)).any() and np.array_equal(got[2].cpu().numpy(), cover(c))
    with pytest.raises(ValueError, match="needs a target"):
        edit_inputs.edit_region_masks(["move"], [a], [None], H, W, DEV)
