"""IP-Adapter Plus on the GPU against the reference (tests/golden/ip_plus_tiny.npz, tools/make_golden.py golden_ip_plus): the Resampler as
TrunkPlan.record_resampler records it, and the tiny UNet with Plus adapters - one image (T = 16), two images (T = 32), a Plus and a base
adapter together - at the bar tests/test_ip_adapter_gpu.py holds the base adapter to (rel_err < 1e-2 and PSNR > 40 dB)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import clip_vision_common as cv  # noqa: E402
from tests import ip_adapter_common as ip  # noqa: E402

DEV = torch.device("cuda:0")
rel_err = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())


@pytest.fixture(scope="module")
def zp(golden_dir):
    return np.load(os.path.join(golden_dir, "ip_plus_tiny.npz"))


def _device_adapter(sd):
    from blobctrl_amd.weights import convert_ip_adapter, ip_adapter_on_device, ip_attn2_prefixes
    from tests.common import TINY, tiny_weights
    return ip_adapter_on_device(convert_ip_adapter(sd, ip_attn2_prefixes(tiny_weights()[0].keys()), TINY["ctx"]), DEV)


@pytest.mark.parametrize("spelling", ("original", "converted"))
@pytest.mark.parametrize("kind", sorted(cv.PLUS_QUERIES))
def test_resampler_tokens_match_the_reference(zp, kind, spelling):
    """record_resampler alone in a segment, for one and two images per UNet image, from either key spelling."""
    from blobctrl_amd.engine import IpAdapter, TrunkConfig, TrunkPlan
    from blobctrl_amd.launch import Recorder
    from tests.common import psnr
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    sd = cv.tiny_plus_adapter(kind)
    if spelling == "converted":
        sd = dict(sd, image_proj=cv.plus_converted(sd["image_proj"]))
    ad = _device_adapter(sd)
    for name, (B, n) in cv.PLUS_TOKEN_SHAPES.items():
        rec = Recorder(DEV)
        try:
            seg = rec.begin("resampler")
            plan = TrunkPlan.__new__(TrunkPlan)
            plan.rec, plan.B = rec, B
            adapter, buf = IpAdapter.for_plan(rec, ad, B, (n, cv.PLUS_SEQ))
            tokens = plan.record_resampler(adapter)
            buf.copy_(cv.plus_hidden(name).reshape(buf.shape).to(DEV, torch.float16))
            seg.run(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got, ref = tokens.float().cpu().numpy(), zp[f"tokens_{kind}_{name}"]
            print(f"resampler {kind} {name} ({spelling}): rel {rel_err(got, ref):.3e}, PSNR {psnr(got, ref):.1f} dB")
            assert got.shape == ref.shape and rel_err(got, ref) < 1e-2 and psnr(got, ref) > 40.0
            assert dict(seg.kinds)["attention"] == 4
        finally:
            rec.close()


@pytest.mark.parametrize("case", sorted(cv.PLUS_UNET_CASES))
def test_unet_module_matches_the_reference_with_plus_adapters(zp, case, monkeypatch):
    """UNet2DConditionModel.load_ip_adapter_weights with Plus adapters (original key spelling) + forward(added_cond_kwargs={"image_embeds":
    [4D hidden states ...]}).  Scale 0 is bit-identical to the same plan run again at scale 0 and within the bar of the reference's
    adapter-less eps; a change of scale records no new plan; after unload the module is bit-identical to one that never loaded one."""
    from blobctrl_amd.modules import UNet2DConditionModel
    from tests.common import g, psnr, set_plan, tiny_weights
    from tests.gpu_common import tiny_trunk_configs
    z = zp
    geo, adapters = cv.PLUS_UNET_CASES[case]
    x, ehs, seed, ins = cv.plus_unet_inputs(case)
    x, ehs, ins = x.to(DEV), ehs.to(DEV), [e.to(DEV) for e in ins]
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
    unet.load_ip_adapter_weights(cv.plus_unet_adapters(case))
    assert unet.config.encoder_hid_dim_type == "ip_image_proj"
    outs = {}
    for what, f in (("eps", 1.0), ("eps_other_scale", float(z["other_factor"])), ("eps_off", 0.0)):
        unet.set_ip_adapter_scale([f * s for s in cv.PLUS_UNET_SCALES[case]])
        got, ref = run(unet, added_cond_kwargs={"image_embeds": ins}), z[f"{case}_{what}"]
        outs[what] = got
        print(f"IP-Adapter Plus UNet {case} {what}: rel {rel_err(got, ref):.3e}, PSNR {psnr(got, ref):.1f} dB; vs eps_off {rel_err(ref, z[f'{case}_eps_off']):.3f}")
        assert rel_err(got, ref) < 1e-2 and psnr(got, ref) > 40.0, what
        assert len(unet._plans) == 1                                           # the scales are no part of the plan key
    assert rel_err(outs["eps"], outs["eps_off"]) > 0.1                        # (the adapter is seen: the reference's gap is 35 bars and more)
    seg = next(iter(unet._plans.values())).seg
    n_plus = sum(kind != "base" for kind, _ in adapters)
    tokens = sorted({m["shape"][-1] for m in seg.meta if m["kind"] == "attention_ip"})
    want = sorted({(4 if kind == "base" else cv.PLUS_QUERIES[kind]) * n for kind, n in adapters})
    assert seg.kinds["attention_ip"] == 16 * len(adapters) and seg.kinds["ip_kv"] == 32 * len(adapters) and tokens == want, (seg.kinds, tokens)
    assert seg.kinds.get("ip_proj", 0) == len(adapters) - n_plus and seg.kinds["ip_resampler"] == 22 * n_plus
    # scale 0: the launches return before they touch anything, so the plan with the adapter-less forms of attn2 is what runs - twice the same
    assert np.array_equal(run(unet, added_cond_kwargs={"image_embeds": ins}), outs["eps_off"])
    with pytest.raises(ValueError, match="Plus"):
        run(unet, added_cond_kwargs={"image_embeds": [e[:, :, 0] if e.ndim == 4 else e for e in ins]})
    unet.unload_ip_adapter()
    assert unet.config.encoder_hid_dim_type is None and not unet._plans
    assert np.array_equal(run(unet), run(never))
    # ... and bit-identical to the adapter-less plan on the attn2 forms that store q (BC_PLAN midx=0 ctx_fold=0), which an adapter plan takes
    set_plan(monkeypatch, midx=0, ctx_fold=0)
    unfused = UNet2DConditionModel(tiny_weights()[0], tiny_trunk_configs()[0])
    assert np.array_equal(run(unfused), outs["eps_off"])
