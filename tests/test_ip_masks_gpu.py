"""IP-Adapter masks on the GPU: bc_attention_ip_masked alone against float64 in NaN-fenced buffers, bc_ip_mask_downsample against its
float64 restatement and the reference's outputs, and blocks, the tiny UNet and the pipeline's `__call__` with
cross_attention_kwargs={"ip_adapter_masks": ...} against the reference's fixtures (tests/ip_masks_common.py: inputs, references, cases).
The masked launch is held to the attention bar of tests/attention_common.py, the bar of the unmasked launch: it rounds once, at the fp16
store, and what it adds - the weight m[i, r] / l_i and the sum over images - is fp32."""
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import attention_common as ac  # noqa: E402
from tests import ip_adapter_common as ipc  # noqa: E402
from tests import ip_masks_common as mc  # noqa: E402

DEV = torch.device("cuda:0")


def _ptr(x):
    return x.data_ptr() if torch.is_tensor(x) else x


def launch(prob, path=None):
    """path None: through the Recorder as the planner records it (the dispatcher's choice); 0 / 1: bc_attention_ip_masked_with by name."""
    from blobctrl_amd import _lib
    from blobctrl_amd.launch import Recorder
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    prob.assert_inside()
    prob.o.snapshot()
    if path is not None:
        _lib.check(_lib.load().bc_attention_ip_masked_with(path, *[_ptr(a) for a in prob.args()], torch.cuda.current_stream().cuda_stream),
                   f"bc_attention_ip_masked_with({path})")
        torch.cuda.synchronize()
        return None
    rec = Recorder(DEV)
    try:
        seg = rec.begin("launch")
        rec.attention_ip_masked(*prob.args())
        seg.run(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return dict(seg.kinds)
    finally:
        rec.close()


def _bits(x):
    return x.half().view(torch.int16)


def _paths(prob):
    """The kernels that take the shape, by name: the scalar one always, the MFMA tiles where Tp is a multiple of 16 (whatever the
    dispatcher would pick for the shape)."""
    return (0, 1) if prob.Tp % 16 == 0 else (0,)


@pytest.mark.parametrize("heads,d,images,Tp", [hd + it for it in mc.IMAGES_TP for hd in mc.HEADS_D] +
                         [hd + it for it in mc.IMAGES_TP_MORE for hd in mc.HEADS_D_MORE])
def test_masked_attention_against_float64(heads, d, images, Tp):
    """Every (heads, d) x (images, Tp), and the head sizes 16, 32 and 64 at (3, 5) and (2, 16), at B = 2 x 72 rows, ldq = 2 C, for
    w = 1, 0.35 and -0.5, by the dispatcher and by every path that takes the shape: within the attention bar, no non-finite element in
    the view, every bit outside the view as it was; rows whose mask is zero for every image - a whole row block, and all but one row of
    the last block - come back bit-identical."""
    for w in mc.WEIGHTS:
        for path in (None,) + _paths(mc.Problem("cpu", heads, d, images, Tp, w)):
            prob = mc.Problem(DEV, heads, d, images, Tp, w)
            q, k, v, o, mask, _ = prob.cpu
            power = mc.mask_power(q, k, v, o, mask, heads, d, images, Tp, w)
            assert min(power.values()) >= 0.5, power
            kinds = launch(prob, path)
            assert kinds in (None, {"attention_ip_masked": 1})
            what = f"attention_ip_masked heads={heads} d={d} images={images} Tp={Tp} w={w} path={'dispatch' if path is None else path}"
            vals, fenced = prob.o.check(what)
            err = ((vals - prob.ref).abs() / ac.bar(prob.ref)).max().item()
            print(f"MARGIN {what}: max err/bar {err:.3f}, {fenced} fence elements untouched; wrong uses seen on {power}")
            assert fenced > 0 and err <= 1.0, f"{what}: max err/bar {err:.3f}"
            for region in ("zero", "single_zero"):
                rows = prob.rows_of(region)
                assert torch.equal(_bits(vals[rows]), _bits(prob.o_in[rows])), f"{what}: rows of the {region} region were rewritten"
            moved = (vals[prob.rows_of("single")] != prob.o_in[prob.rows_of("single")].double()).any(-1)
            assert bool(moved.all()), f"{what}: the one non-zero row of the last block was skipped"


@pytest.mark.parametrize("heads,d,images,Tp", [(2, 8, 1, 4), (8, 40, 2, 4), (8, 160, 4, 16)])
def test_masked_attention_zero_weight_touches_nothing(heads, d, images, Tp):
    """w == 0: the reference skips the adapter; O and its fences are bit-identical after the launch."""
    prob = mc.Problem(DEV, heads, d, images, Tp, 0.0)
    assert launch(prob) == {"attention_ip_masked": 1}
    assert prob.o.untouched()


# ---------------------------------------------------------------------------------------------------- the downsampling
@pytest.fixture(scope="module")
def zd(golden_dir):
    return np.load(os.path.join(golden_dir, "ip_mask_downsample.npz"))


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("H,W,rows", mc.DOWNSAMPLE_CASES)
def test_downsample_against_float64_and_the_reference(zd, H, W, rows, u8):
    """bc_ip_mask_downsample from fp32 and from uint8 masks into a NaN-fenced fp16 buffer [2][rows + 8]: at most one fp16 rounding of the
    float64 value (2^-11 |v|) plus 1e-6 from the float64 restatement, and from the reference's own output; a padded tail exactly zero;
    the fence intact."""
    from blobctrl_amd import ip_masks
    from tests import norm_layout_common as nl
    m = mc.downsample_masks(H, W)
    ref64 = ip_masks.downsample_reference(m, rows)
    dev_mask = torch.from_numpy(m if u8 else m.astype(np.float32)).to(DEV)
    out = nl.InPlace(nl.fence(torch.zeros(2, rows).half(), DEV, ld=(rows + 15) // 8 * 8, guard=1))
    out.assert_inside()
    out.v.valid().fill_(float("nan"))                                          # (the launch writes every element of the view)
    out.snapshot()
    view = out.t.as_strided((2, rows), (out.ld, 1))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        assert ip_masks.downsample(dev_mask, rows, out=view) is view
    torch.cuda.synchronize()
    assert bool(caught) == ((H, W, rows) in mc.DOWNSAMPLE_PADDED)
    what = f"ip_mask_downsample {H} x {W} -> {rows} rows ({'uint8' if u8 else 'fp32'})"
    vals, fenced = out.check(what)
    mh, mw = mc.DOWNSAMPLE_GRIDS[(H, W, rows)]
    for name, ref in (("float64", torch.from_numpy(ref64)), ("reference", torch.from_numpy(zd[f"{H}x{W}_{rows}"]).double())):
        err = ((vals - ref).abs() / (2.0 ** -11 * ref.abs() + 1e-6)).max().item()
        print(f"MARGIN {what} vs {name}: max err/bound {err:.3f}, range [{float(vals.min()):.3f}, {float(vals.max()):.3f}], {fenced} fence elements")
        assert err <= 1.0, f"{what} vs {name}: max err/bound {err:.3f}"
    assert fenced > 0 and not vals[:, mh * mw:].any() and not torch.signbit(vals[:, mh * mw:]).any()


# ---------------------------------------------------------------------------------------------------- one block per planner form
@pytest.fixture(scope="module")
def zb(golden_dir):
    return np.load(os.path.join(golden_dir, "blocks_ip_masks.npz"))


def _rel(got, ref, sub=1):
    got = got[:, :, ::sub, ::sub] if sub > 1 else got
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("name,form", [("ip_320", "rowchain"), ("ip_320", "unfused"), ("ip_640", "rowchain"), ("ip_1280", "gw")])
def test_block_with_masks(zb, name, form, monkeypatch):
    """The reference's Transformer2DModel with IPAdapterAttnProcessor2_0 and ip_adapter_masks (tests/golden/blocks_ip_masks.npz) against
    the block as TrunkPlan records it for masks, in each planner form, at the bar of tests/test_blocks_gpu.py.  The reference's unmasked
    and swapped-mask outputs lie outside that bar of what the launch gives; after the masks are exchanged on the device the SAME segment
    gives the swapped output."""
    from blobctrl_amd import ip_masks
    from tests.common import set_plan
    from tests.test_blocks_gpu import _check, _nchw, _run
    if form == "unfused":
        set_plan(monkeypatch, rowchain=0, gw=0)
    p = ipc.IP_BLOCK_CASES[name]
    rec, seg, out, adapters = mc.ip_block_plan_masked(name, DEV)
    try:
        kinds, variants = seg.kinds, [m.get("variant", "") for m in seg.meta]
        assert ("rowchain" in kinds) == (form == "rowchain") and any("gemm_wreg_kernel" in v for v in variants) == (form == "gw"), variants
        assert kinds["attention_ip_masked"] == len(p["tokens"]) and "attention_ip" not in kinds, kinds
        masks, n = mc.block_masks(name), len(seg)
        with warnings.catch_warnings():
            warnings.simplefilter("error")                                    # the masks have the canvas' aspect ratio: nothing pads
            ip_masks.fill_plan_masks(adapters, masks, DEV)
        _run(seg)
        got = _nchw(out, p["B"])
        _check(f"{name}_masked ({form})", got, zb[name + "_masked"], p["sub"])
        others = ["_unmasked"] + (["_swapped"] if mc.block_has_swap(name) else [])
        for tag in others:
            gap = _rel(got, zb[name + tag], p["sub"])
            print(f"block {name}_masked ({form}) vs the reference's {tag}: max-abs/scale {gap:.3f}")
            assert gap > 1e-2, tag
        if mc.block_has_swap(name):
            ip_masks.fill_plan_masks(adapters, mc.swap_images(masks), DEV)
            _run(seg)
            _check(f"{name}_swapped ({form})", _nchw(out, p["B"]), zb[name + "_swapped"], p["sub"])
        assert len(seg) == n                                                  # nothing was recorded again
    finally:
        rec.close()


# ---------------------------------------------------------------------------------------------------- the tiny UNet module
@pytest.mark.parametrize("case", sorted(ipc.IP_UNET_CASES))
def test_unet_module_with_masks_matches_the_reference(golden_dir, case):
    """UNet2DConditionModel.forward(cross_attention_kwargs={"ip_adapter_masks": [...]}) against the reference's forward
    (tests/golden/unet_tiny_ip_masks.npz), masks at the image resolution, at the bar tests/test_freeu_gpu.py holds the same UNet to.
    Other masks replay the masked plan; a call without masks takes the unmasked plan and gives unet_tiny_ip.npz's eps."""
    from blobctrl_amd.modules import UNet2DConditionModel
    from tests.common import g, psnr, tiny_weights
    from tests.gpu_common import tiny_trunk_configs
    z = np.load(os.path.join(golden_dir, "unet_tiny_ip.npz"))
    zm = np.load(os.path.join(golden_dir, "unet_tiny_ip_masks.npz"))
    geo, images = ipc.IP_UNET_CASES[case]
    x, ehs, seed, embeds = ipc.ip_unet_inputs(case)
    x, ehs, embeds = x.to(DEV), ehs.to(DEV), [e.to(DEV) for e in embeds]
    B, _, H, W = x.shape
    unet = UNet2DConditionModel(tiny_weights()[0], tiny_trunk_configs()[0])

    def res(m):
        down, mid, up = m._res_shapes(H, W)
        sq = lambda s: (s[0], s[1], min(s[1], s[2]))
        mk = lambda i, s: (g(seed + i, B, *sq(s)) * float(z["res_scale"])).to(DEV)
        return dict(down_block_add_samples=[mk(i, s) for i, s in enumerate(down)], mid_block_add_sample=mk(100, mid),
                    up_block_add_samples=[mk(200 + i, s) for i, s in enumerate(up)])

    def run(masks=None, **extra):
        kw = {} if masks is None else dict(cross_attention_kwargs={"ip_adapter_masks": masks, **extra})
        return unet(x, int(z["timestep"]), encoder_hidden_states=ehs, return_dict=False, added_cond_kwargs={"image_embeds": embeds},
                    **res(unet), **kw)[0].cpu().numpy()
    rel_err = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    unet.load_ip_adapter_weights([ipc.tiny_ip_adapter(i) for i in range(len(images))])
    unet.set_ip_adapter_scale(list(ipc.IP_UNET_SCALES[case]))
    masks = mc.unet_masks(case)
    variants = [("eps_masked", masks)] + ([("eps_swapped", mc.swap_images(masks))] if any(n > 1 for n in images) else [])
    for what, mk in variants:
        got, ref = run([m.to(DEV) for m in mk] if what == "eps_masked" else mk), zm[f"{case}_{what}"]       # device masks, then host masks
        print(f"IP-Adapter masks UNet {case} {what}: rel {rel_err(got, ref):.3e}, PSNR {psnr(got, ref):.1f} dB; "
              f"vs unmasked {rel_err(ref, z[f'{case}_eps']):.3f}")
        assert rel_err(got, ref) < 1e-2 and psnr(got, ref) > 40.0, what
        assert len(unet._plans) == 1                                          # the masks are no part of the plan key
    (key, P), = unet._plans.items()
    assert key[-1] == ("ip", "masked") and P.seg.kinds["attention_ip_masked"] == 16 * len(images) and "attention_ip" not in P.seg.kinds
    first = run(masks)
    assert np.array_equal(run([m.to(torch.uint8).to(DEV) for m in masks]), first) and len(unet._plans) == 1      # uint8 0 / 1: the same values
    plain = run()
    assert len(unet._plans) == 2 and rel_err(plain, z[f"{case}_eps"]) < 1e-2 and psnr(plain, z[f"{case}_eps"]) > 40.0
    assert "attention_ip_masked" not in list(unet._plans.values())[-1].seg.kinds
    with pytest.raises(ValueError, match="foo"):
        run(masks, foo=1)


# ---------------------------------------------------------------------------------------------------- __call__
def test_pipeline_call_with_masks_matches_the_reference_call(golden_dir):
    """The reference's own `__call__` with an IP-Adapter and cross_attention_kwargs={"ip_adapter_masks": [...]}
    (tests/golden/pipeline_call_ip_masks.npz: DDIM, 3 steps, classifier-free guidance, two images per prompt), with the whole-edit graph
    on, at the bar of tests/test_freeu_gpu.py's pipeline case: mask A; mask B on the same plan and the same captured graph; no masks, on
    the unmasked plan, as pipeline_call_ip.npz has it; and a uint8 device mask from edit_inputs.ellipse_masks, which gives the latents
    the same mask gives as a PIL image, bit for bit.  Without an adapter the key is ignored."""
    from PIL import Image
    from blobctrl_amd import edit_inputs
    from blobctrl_amd.clip_text import CLIPTextModel
    from blobctrl_amd.dinov2 import Dinov2Model
    from blobctrl_amd.image_processor import IPAdapterMaskProcessor
    from blobctrl_amd.modules import BlobNetModel, UNet2DConditionModel
    from blobctrl_amd.pipeline import StableDiffusionBlobNetPipeline
    from blobctrl_amd.schedulers import DDIMScheduler
    from blobctrl_amd.vae import AutoencoderKL
    from tests.common import PIPE, FakeTokenizer, pipeline_cases, psnr, tiny_pipeline_weights, tiny_weights
    from tests.gpu_common import tiny_trunk_configs
    from tests.test_freeu_gpu import SD
    z = np.load(os.path.join(golden_dir, "pipeline_call.npz"))
    zi = np.load(os.path.join(golden_dir, "pipeline_call_ip.npz"))
    zm = np.load(os.path.join(golden_dir, "pipeline_call_ip_masks.npz"))
    rel_err = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    vsd, csd, dsd = tiny_pipeline_weights()
    usd, bsd = tiny_weights()
    ucfg, bcfg = tiny_trunk_configs()
    pipe = StableDiffusionBlobNetPipeline(
        tokenizer=FakeTokenizer(), scheduler=DDIMScheduler(**SD), safety_checker=None, requires_safety_checker=False, use_graphs=True,
        unet=UNet2DConditionModel(usd, ucfg), blobnet=BlobNetModel(bsd, bcfg), vae=AutoencoderKL(vsd, norm_num_groups=PIPE["vae_groups"]),
        text_encoder=CLIPTextModel(csd, num_heads=PIPE["clip"]["heads"]),
        dinov2=Dinov2Model(dsd, num_heads=PIPE["dino"]["heads"], patch_size=PIPE["dino"]["patch"]))
    kw = dict(pipeline_cases()["ddim_neg2"])
    for k in ("scheduler", "seed", "rng_seed", "num_inference_steps"):
        kw.pop(k)
    seed, rng_seed, steps = int(zi["seed"]), int(zi["rng_seed"]), int(zi["num_inference_steps"])
    embeds = torch.from_numpy(zi["embeds"])
    common = dict(fg_image=Image.fromarray(z["fg"]), bg_image=Image.fromarray(z["bg"]), gs_score=torch.from_numpy(z["gs_score"]),
                  height=64, width=64, output_type="latent", num_inference_steps=steps, **kw)

    def call(masks=None, **extra):
        torch.manual_seed(rng_seed)
        ck = {} if masks is None else dict(cross_attention_kwargs={"ip_adapter_masks": masks})
        return pipe(generator=torch.Generator().manual_seed(seed), **common, **ck, **extra).images.cpu().numpy()
    mp = IPAdapterMaskProcessor()

    def pre(image):
        m = mp.preprocess(image, height=64, width=128)
        return [m.reshape(1, m.shape[0], m.shape[2], m.shape[3])]
    # no adapter: the key is ignored, silently
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        plain = call()
        assert np.array_equal(call(pre(Image.fromarray(zm["mask_A"]))), plain)
    pipe.load_ip_adapter(ipc.tiny_ip_adapter(0))
    pipe.set_ip_adapter_scale(ipc.IP_CALL_SCALE)
    ip_kw = dict(ip_adapter_image_embeds=[embeds])
    # mask A
    masks_a = pre(Image.fromarray(zm["mask_A"]))
    assert np.array_equal(masks_a[0].numpy(), zm["pre_A"])
    got_a = call(masks_a, **ip_kw)
    eng = pipe.engine
    print(f"__call__ ip-adapter masks, A: max-abs/scale {rel_err(got_a, zm['latents_A']):.3e}, PSNR {psnr(got_a, zm['latents_A']):.1f} dB; "
          f"reference A vs B {rel_err(zm['latents_A'], zm['latents_B']):.3f}, A vs none {rel_err(zm['latents_A'], zm['latents_none']):.3f}")
    assert rel_err(got_a, zm["latents_A"]) < 1e-2 and psnr(got_a, zm["latents_A"]) > 40.0
    key = list(eng._plans)[-1]
    assert eng.loop_graph and key[-1] == ("ip", "masked", 1) and key[-2] == ("ip", 1, (4, ipc.IP_EMBED_DIM))
    P = eng._plans[key]
    graphs = dict(P.loop_graphs)
    assert len(graphs) == 1
    # mask B: the same plan, the same whole-edit graph, nothing recorded or captured
    st, plans = dict(eng.cache_stats), len(eng._plans)
    got_b = call(pre(Image.fromarray(zm["mask_B"])), **ip_kw)
    st2 = eng.cache_stats
    assert len(eng._plans) == plans and list(eng._plans)[-1] == key and eng._plans[key] is P
    assert st2["plans_recorded"] == st["plans_recorded"] and st2["loop_graph_captures"] == st["loop_graph_captures"]
    assert st2["plan_hits"] == st["plan_hits"] + 1 and st2["loop_graph_hits"] == st["loop_graph_hits"] + 1
    assert dict(P.loop_graphs) == graphs                                          # the same graph object under the same pattern
    print(f"__call__ ip-adapter masks, B: max-abs/scale {rel_err(got_b, zm['latents_B']):.3e}; vs A {rel_err(got_b, got_a):.3f}")
    assert rel_err(got_b, zm["latents_B"]) < 1e-2 and psnr(got_b, zm["latents_B"]) > 40.0 and rel_err(got_b, got_a) > 0.1
    # without masks: the unmasked plan, pipeline_call_ip.npz's latents
    none = call(**ip_kw)
    assert len(eng._plans) == plans + 1 and list(eng._plans)[-1][-1] == ("ip", 1, (4, ipc.IP_EMBED_DIM))
    assert np.array_equal(zm["latents_none"], zi["latents"]) and rel_err(none, zi["latents"]) < 1e-2 and psnr(none, zi["latents"]) > 40.0
    # a uint8 device mask (an edit's own blob ellipse, 255 / 0 on a 128 x 256 frame) through the device route, and the same pixels as a PIL image
    ellipse = ((170.0, 66.0), (90.0, 60.0), 25.0)
    dev_mask = edit_inputs.ellipse_masks([ellipse], 128, 256, device=DEV)
    masks_dev = pre(dev_mask[0])
    masks_pil = pre(Image.fromarray(dev_mask[0].cpu().numpy()))
    assert masks_dev[0].is_cuda and masks_dev[0].dtype == torch.uint8 and tuple(masks_dev[0].shape) == (1, 1, 64, 128)
    assert np.array_equal(masks_dev[0].cpu().numpy().astype(np.float32), masks_pil[0].numpy()) and 0.05 < float(masks_pil[0].mean()) < 0.5
    st = dict(eng.cache_stats)
    got_dev, got_pil = call(masks_dev, **ip_kw), call(masks_pil, **ip_kw)
    assert np.array_equal(got_dev, got_pil) and rel_err(got_dev, none) > 0.1 and eng.cache_stats["plans_recorded"] == st["plans_recorded"]
    # the checks of the processor, with its wording
    with pytest.raises(ValueError, match="Number of masks"):
        call([torch.zeros(1, 2, 64, 128)], **ip_kw)
    with pytest.raises(ValueError, match="Length of ip_adapter_masks array"):
        call(masks_a + masks_a, **ip_kw)
    with pytest.raises(ValueError, match="foo"):
        torch.manual_seed(rng_seed)
        pipe(generator=torch.Generator().manual_seed(seed), **common, **ip_kw, cross_attention_kwargs={"ip_adapter_masks": masks_a, "foo": 1})
