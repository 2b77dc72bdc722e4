"""bc_attention_ip (csrc/attention_ip.hip) alone against float64, in NaN-fenced buffers (tests/ip_adapter_common.py: inputs, reference,
fences).  The launch goes through the Recorder as the planner records it - Recorder.attention_ip, one launch per segment, replayed once.
Bar: the project's attention bar (tests/attention_common.py) around O_in + w * attn64 computed from the launch's own fp16 inputs.
Before a launch the test checks its own inputs on the CPU: the float64 result with one key dropped, and with one key taken from the
other image, must leave the bar on at least half of the rows - otherwise the inputs could not see a wrong key set."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import attention_common as ac  # noqa: E402
from tests import ip_adapter_common as ip  # noqa: E402

DEV = torch.device("cuda:0")


def launch(prob):
    from blobctrl_amd.launch import Recorder
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    prob.assert_inside()
    prob.o.snapshot()
    rec = Recorder(DEV)
    try:
        seg = rec.begin("launch")
        rec.attention_ip(*prob.args())
        seg.run(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return dict(seg.kinds)
    finally:
        rec.close()


@pytest.mark.parametrize("T", ip.TOKENS)
@pytest.mark.parametrize("d", ip.HEAD_DIMS)
@pytest.mark.parametrize("heads", ip.HEADS)
def test_attention_ip_against_float64(heads, d, T):
    """Every (heads, d, T) at B = 2 x 72 rows (a ragged last row block, a block boundary at the image boundary), ldq = 2 C, for w = 1, 0.35
    and -0.5: within the attention bar, no non-finite element in the view, every bit outside the view as it was."""
    for w in ip.WEIGHTS:
        prob = ip.Problem(DEV, heads, d, T, w)
        q, k, v, o = prob.cpu
        power = ip.key_set_power(q, k, v, o, heads, d, w)
        print(f"attention_ip heads={heads} d={d} T={T} w={w}: rows that see a wrong key set {power}")
        assert power and min(power.values()) >= 0.5, power
        assert launch(prob) == {"attention_ip": 1}
        what = f"attention_ip heads={heads} d={d} T={T} w={w}"
        vals, fenced = prob.o.check(what)
        err = ((vals - prob.ref).abs() / ac.bar(prob.ref)).max().item()
        print(f"MARGIN {what}: max err/bar {err:.3f}, {fenced} fence elements untouched")
        assert fenced > 0 and err <= 1.0, f"{what}: max err/bar {err:.3f}"


@pytest.mark.parametrize("heads,d,T", [(2, 8, 1), (8, 40, 4), (8, 160, 64)])
def test_attention_ip_zero_weight_touches_nothing(heads, d, T):
    """w == 0: the reference skips the adapter; O and its fences are byte-identical after the launch."""
    prob = ip.Problem(DEV, heads, d, T, 0.0)
    assert launch(prob) == {"attention_ip": 1}
    assert prob.o.untouched()


# ---------------------------------------------------------------------------------------------------- one block with the IP processor
@pytest.fixture(scope="module")
def zb(golden_dir):
    import os
    import numpy as np
    return np.load(os.path.join(golden_dir, "blocks_ip.npz"))


@pytest.mark.parametrize("name,form", [("ip_320", "rowchain"), ("ip_320", "unfused"), ("ip_640", "rowchain"), ("ip_1280", "gw")])
def test_block_with_ip_adapters(zb, name, form, monkeypatch):
    """The reference's Transformer2DModel with IPAdapterAttnProcessor2_0 on attn2 (tests/golden/blocks_ip.npz) against the block as
    TrunkPlan records it with adapters loaded, in each form - asserted from the launch listing - and at the bar of tests/test_blocks_gpu.py.
    The SAME segment is then replayed after the scale words are rewritten on the device: half the scales, then zero (the launch skips)."""
    from tests.common import set_plan
    from tests.test_blocks_gpu import _check, _nchw, _run
    if form == "unfused":
        set_plan(monkeypatch, rowchain=0, gw=0)
    p = ip.IP_BLOCK_CASES[name]
    rec, seg, out, tables = ip.ip_block_plan(name, DEV)
    try:
        kinds, variants = seg.kinds, [m.get("variant", "") for m in seg.meta]
        assert ("rowchain" in kinds) == (form == "rowchain") and any("gemm_wreg_kernel" in v for v in variants) == (form == "gw"), variants
        assert kinds["attention_ip"] == len(p["tokens"]) and not any("midx" in v for v in variants) and "ctx_fold" not in kinds, kinds
        n = len(seg)
        for tag, f in (("", 1.0), ("_other", 0.5), ("_off", 0.0)):
            for tab, s in zip(tables, ip.IP_BLOCK_SCALES[name]):
                tab.fill_(f * s)
            _run(seg)
            _check(f"{name}{tag} ({form})", _nchw(out, p["B"]), zb[name + tag], p["sub"])
        assert len(seg) == n                                             # nothing was recorded again
    finally:
        rec.close()


# ---------------------------------------------------------------------------------------------------- the tiny UNet module
@pytest.mark.parametrize("case", sorted(ip.IP_UNET_CASES))
def test_unet_module_matches_the_reference_with_ip_adapters(golden_dir, case):
    """UNet2DConditionModel.load_ip_adapter_weights + forward(added_cond_kwargs={"image_embeds": [...]}) against the reference's
    `_load_ip_adapter_weights` forward (tests/golden/unet_tiny_ip.npz), at the bar tests/test_freeu_gpu.py holds the same UNet to.  Scale 0
    with the adapter loaded lies within that bar of eps_off (not bit-equal: the plan takes the unfused attn2 forms); a change of scale
    records no new plan; after unload_ip_adapter the module is bit-identical to one that never loaded an adapter."""
    import os
    import numpy as np
    from blobctrl_amd.modules import UNet2DConditionModel
    from tests.common import g, psnr, tiny_weights
    from tests.gpu_common import tiny_trunk_configs
    z = np.load(os.path.join(golden_dir, "unet_tiny_ip.npz"))
    rel_err = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    geo, images = ip.IP_UNET_CASES[case]
    x, ehs, seed, embeds = ip.ip_unet_inputs(case)
    x, ehs, embeds = x.to(DEV), ehs.to(DEV), [e.to(DEV) for e in embeds]
    B, _, H, W = x.shape
    unet = UNet2DConditionModel(tiny_weights()[0], tiny_trunk_configs()[0])
    never = UNet2DConditionModel(tiny_weights()[0], tiny_trunk_configs()[0])

    def res(m):
        down, mid, up = m._res_shapes(H, W)
        sq = lambda s: (s[0], s[1], min(s[1], s[2]))
        mk = lambda i, s: (g(seed + i, B, *sq(s)) * float(z["res_scale"])).to(DEV)
        return dict(down_block_add_samples=[mk(i, s) for i, s in enumerate(down)], mid_block_add_sample=mk(100, mid),
                    up_block_add_samples=[mk(200 + i, s) for i, s in enumerate(up)])
    run = lambda m, **kw: m(x, int(z["timestep"]), encoder_hidden_states=ehs, return_dict=False, **res(m), **kw)[0].cpu().numpy()
    assert unet.config.encoder_hid_dim_type is None
    unet.load_ip_adapter_weights([ip.tiny_ip_adapter(i) for i in range(len(images))])
    assert unet.config.encoder_hid_dim_type == "ip_image_proj"
    with pytest.raises(ValueError, match="image_embeds"):
        run(unet)
    plans = None
    for what, f in (("eps", 1.0), ("eps_other_scale", float(z["other_factor"])), ("eps_off", 0.0)):
        unet.set_ip_adapter_scale([f * s for s in ip.IP_UNET_SCALES[case]])
        got, ref = run(unet, added_cond_kwargs={"image_embeds": embeds}), z[f"{case}_{what}"]
        print(f"IP-Adapter UNet {case} {what}: rel {rel_err(got, ref):.3e}, PSNR {psnr(got, ref):.1f} dB; vs eps_off {rel_err(ref, z[f'{case}_eps_off']):.3f}")
        assert rel_err(got, ref) < 1e-2 and psnr(got, ref) > 40.0, what
        plans = len(unet._plans) if plans is None else plans
        assert len(unet._plans) == plans == 1                                  # the scales are no part of the plan key
    kinds = next(iter(unet._plans.values())).seg.kinds
    assert kinds["attention_ip"] == 16 * len(images) and kinds["ip_proj"] == len(images) and kinds["ip_kv"] == 32 * len(images), kinds
    unet.unload_ip_adapter()
    assert unet.config.encoder_hid_dim_type is None and not unet._plans
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        run(unet, added_cond_kwargs={"image_embeds": embeds})
    assert np.array_equal(run(unet), run(never))
    assert "attention_ip" not in next(iter(unet._plans.values())).seg.kinds


# ---------------------------------------------------------------------------------------------------- __call__
def test_pipeline_call_with_an_ip_adapter_matches_the_reference_call(golden_dir):
    """The reference's own `__call__` with an IP-Adapter loaded and `ip_adapter_image_embeds` given (tests/golden/pipeline_call_ip.npz:
    classifier-free guidance, two images per prompt, DDIM, 3 steps), keyword for keyword with the whole-edit graph on, at the bar of
    tests/test_freeu_gpu.py's pipeline case.  A second call after set_ip_adapter_scale matches `latents_other` on the same plan and the
    same captured graph; the eager path agrees bit for bit; a batch that does not fit the UNet batch is a ValueError; after
    unload_ip_adapter the latents are bit-identical to those of a pipeline that never loaded an adapter, and they are the reference's."""
    import os
    import numpy as np
    from PIL import Image
    from blobctrl_amd.clip_text import CLIPTextModel
    from blobctrl_amd.dinov2 import Dinov2Model
    from blobctrl_amd.modules import BlobNetModel, UNet2DConditionModel
    from blobctrl_amd.pipeline import StableDiffusionBlobNetPipeline
    from blobctrl_amd.schedulers import DDIMScheduler
    from blobctrl_amd.vae import AutoencoderKL
    from tests.common import PIPE, FakeTokenizer, pipeline_cases, psnr, tiny_pipeline_weights, tiny_weights
    from tests.gpu_common import tiny_trunk_configs
    from tests.test_freeu_gpu import SD
    z = np.load(os.path.join(golden_dir, "pipeline_call.npz"))
    zi = np.load(os.path.join(golden_dir, "pipeline_call_ip.npz"))
    rel_err = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    vsd, csd, dsd = tiny_pipeline_weights()

    def mk(graphs=True):
        usd, bsd = tiny_weights()
        ucfg, bcfg = tiny_trunk_configs()
        return StableDiffusionBlobNetPipeline(
            tokenizer=FakeTokenizer(), scheduler=DDIMScheduler(**SD), safety_checker=None, requires_safety_checker=False, use_graphs=graphs,
            unet=UNet2DConditionModel(usd, ucfg), blobnet=BlobNetModel(bsd, bcfg), vae=AutoencoderKL(vsd, norm_num_groups=PIPE["vae_groups"]),
            text_encoder=CLIPTextModel(csd, num_heads=PIPE["clip"]["heads"]),
            dinov2=Dinov2Model(dsd, num_heads=PIPE["dino"]["heads"], patch_size=PIPE["dino"]["patch"]))
    kw = dict(pipeline_cases()["ddim_neg2"])
    for k in ("scheduler", "seed", "rng_seed", "num_inference_steps"):
        kw.pop(k)
    seed, rng_seed, steps = int(zi["seed"]), int(zi["rng_seed"]), int(zi["num_inference_steps"])
    embeds = torch.from_numpy(zi["embeds"])
    assert np.array_equal(zi["embeds"], ip.ip_call_embeds().numpy())
    common = dict(fg_image=Image.fromarray(z["fg"]), bg_image=Image.fromarray(z["bg"]), gs_score=torch.from_numpy(z["gs_score"]),
                  height=64, width=64, output_type="latent", num_inference_steps=steps, **kw)

    def call(p, **extra):
        torch.manual_seed(rng_seed)
        return p(generator=torch.Generator().manual_seed(seed), **common, **extra).images.cpu().numpy()
    never = mk()
    plain = call(never)
    pipe = mk()
    assert np.array_equal(call(pipe), plain)
    pipe.load_ip_adapter(ip.tiny_ip_adapter(0))
    assert pipe.unet.config.encoder_hid_dim_type == "ip_image_proj"
    pipe.set_ip_adapter_scale(ip.IP_CALL_SCALE)
    got, ref = call(pipe, ip_adapter_image_embeds=[embeds]), zi["latents"]
    eng = pipe.engine
    assert eng.loop_graph and list(eng._plans)[-1][-1] == ("ip", 1, (4, ip.IP_EMBED_DIM)) and len(eng._plans) == 2
    print(f"__call__ ip-adapter: end to end max-abs/scale {rel_err(got, ref):.3e}, PSNR {psnr(got, ref):.1f} dB; "
          f"reference on vs off {rel_err(ref, zi['latents_off']):.3f}")
    assert got.shape == ref.shape and rel_err(got, ref) < 1e-2 and psnr(got, ref) > 40.0
    # another scale: a plan hit, no new plan, no new capture - and the reference's other answer
    st = dict(eng.cache_stats)
    pipe.set_ip_adapter_scale([ip.IP_CALL_SCALE_OTHER])
    got2 = call(pipe, ip_adapter_image_embeds=[embeds])
    st2 = eng.cache_stats
    assert len(eng._plans) == 2 and st2["plans_recorded"] == st["plans_recorded"] and st2["loop_graph_captures"] == st["loop_graph_captures"]
    assert st2["plan_hits"] == st["plan_hits"] + 1 and st2["loop_graph_hits"] == st["loop_graph_hits"] + 1
    print(f"__call__ ip-adapter, other scale: max-abs/scale {rel_err(got2, zi['latents_other']):.3e}; vs the first {rel_err(got2, got):.3f}")
    assert rel_err(got2, zi["latents_other"]) < 1e-2 and psnr(got2, zi["latents_other"]) > 40.0 and rel_err(got2, got) > 0.1
    # the eager path (no graphs) agrees bit for bit
    pipe.set_ip_adapter_scale(ip.IP_CALL_SCALE)
    assert np.array_equal(call(pipe, ip_adapter_image_embeds=[embeds]), got)
    eager = mk(False)
    eager.load_ip_adapter([ip.tiny_ip_adapter(0)])
    assert np.array_equal(call(eager, ip_adapter_image_embeds=[embeds]), got) and eager.engine.cache_stats["loop_graph_captures"] == 0
    # a batch that is not the UNet batch after the chunk and repeat; adapters loaded and no embeddings; both inputs
    with pytest.raises(ValueError, match="UNet batch"):
        call(pipe, ip_adapter_image_embeds=[torch.cat([embeds, embeds], 0)])
    with pytest.raises(ValueError, match="are loaded"):
        call(pipe)
    with pytest.raises(NotImplementedError, match="ip_adapter_image_embeds"):
        call(pipe, ip_adapter_image=Image.fromarray(z["fg"]))
    # unload: the adapter-less plan, bit-identical to a pipeline that never loaded one, and the reference's adapter-less latents
    pipe.unload_ip_adapter()
    off = call(pipe)
    assert len(pipe.engine._plans) == 1 and np.array_equal(off, plain)
    assert rel_err(off, zi["latents_off"]) < 1e-2 and psnr(off, zi["latents_off"]) > 40.0
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        call(pipe, ip_adapter_image_embeds=[embeds])
