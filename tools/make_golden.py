#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REAL reference (imported from /root/reference) on CPU fp32.

Runs only in the build container (needs /root/reference).  Nothing from the reference is copied: the fixtures hold
inputs and expected outputs only.  Weights are NOT stored - both sides regenerate them from
`blobctrl_amd.synth` (numpy PCG64 keyed by parameter name), and this script checks `load_state_dict(strict=True)`
so the parameter schema in `blobctrl_amd/synth.py` is pinned against the reference classes too.

Import recipe: vendored diffusers first, FLAX_WEIGHTS_NAME shim, stub modules for cv2/torchvision.
"""
import json
import os
import sys
import types
import importlib.machinery

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path[:0] = ["/root/reference/diffusers/src", "/root/reference", REPO]

import numpy as np
import torch

import transformers.utils
transformers.utils.FLAX_WEIGHTS_NAME = "flax_model.msgpack"
import diffusers  # noqa: E402  (vendored 0.30.0)
for _name in ["cv2", "torchvision", "torchvision.transforms", "torchvision.transforms.functional",
              "matplotlib", "matplotlib.cm"]:
    try:
        __import__(_name)
    except Exception:
        _m = types.ModuleType(_name)
        _m.__spec__ = importlib.machinery.ModuleSpec(_name, None)
        _m.__path__ = []
        sys.modules[_name] = _m

from diffusers import UNet2DConditionModel, DDIMScheduler, UniPCMultistepScheduler  # noqa: E402
from blobctrl.models.blobnet import BlobNetModel  # noqa: E402
from blobctrl.utils.utils import splat_features  # noqa: E402
from blobctrl.pipelines.pipeline_blobnet import StableDiffusionBlobNetPipeline  # noqa: E402
import scripts.blobctrl_inference as ref_inf  # noqa: E402

from blobctrl_amd import synth  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
os.makedirs(OUT, exist_ok=True)
torch.set_grad_enabled(False)
torch.set_num_threads(8)

# ------------------------------------------------------------------------------------------------ tiny configs
TINY = dict(boc=(16, 32, 64, 64), groups=4, heads=2, ctx=16, feat=8, seed=7)
SD_SCHED = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000,
                steps_offset=1)


def build_tiny(time_cond_proj_dim=None):
    """`time_cond_proj_dim`: the UNet of a distilled LCM model (time_embedding.cond_proj over the guidance-scale embedding)."""
    c = TINY
    unet = UNet2DConditionModel(in_channels=5, out_channels=4, block_out_channels=c["boc"], norm_num_groups=c["groups"],
                                attention_head_dim=c["heads"], cross_attention_dim=c["ctx"], layers_per_block=2,
                                time_cond_proj_dim=time_cond_proj_dim)
    # NB: the reference script leaves unet.config.in_channels = 4 (inf:233-249); only conv_in has 5 inputs.
    blob = BlobNetModel(in_channels=4, conditioning_channels=1 + c["feat"], block_out_channels=c["boc"],
                        norm_num_groups=c["groups"], attention_head_dim=c["heads"], cross_attention_dim=None,
                        layers_per_block=2)
    us = synth.trunk_param_shapes(5, c["boc"], 2, c["ctx"], 4, blobnet=False, time_cond_proj_dim=time_cond_proj_dim)
    bs = synth.trunk_param_shapes(4 + 1 + c["feat"], c["boc"], 2, None, None, blobnet=True)
    assert set(us.keys()) == set(unet.state_dict().keys()), "UNet schema mismatch"
    assert all(tuple(v.shape) == tuple(us[k]) for k, v in unet.state_dict().items()), "UNet shape mismatch"
    assert set(bs.keys()) == set(blob.state_dict().keys()), "BlobNet schema mismatch"
    unet.load_state_dict(synth.synth_state_dict(us, c["seed"]), strict=True)
    blob.load_state_dict(synth.synth_state_dict(bs, c["seed"] + 1), strict=True)
    return unet.eval(), blob.eval()


def check_full_schema():
    """Pin the full-size schema (names + shapes) on the meta device: no memory, no arithmetic."""
    with torch.device("meta"):
        unet = UNet2DConditionModel(in_channels=5, out_channels=4, cross_attention_dim=768, attention_head_dim=8)
        blob = BlobNetModel(in_channels=4, conditioning_channels=1025, cross_attention_dim=None, attention_head_dim=8)
    us = synth.trunk_param_shapes(5, (320, 640, 1280, 1280), 2, 768, 4, blobnet=False)
    bs = synth.trunk_param_shapes(1029, (320, 640, 1280, 1280), 2, None, None, blobnet=True)
    for sh, m, n in ((us, unet, "unet"), (bs, blob, "blobnet")):
        ref = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        assert set(ref.keys()) == set(sh.keys()), n
        assert all(ref[k] == tuple(sh[k]) for k in ref), n
        print(f"full-size {n}: {len(ref)} tensors, {sum(int(np.prod(v)) for v in ref.values())/1e6:.1f} M params - schema OK")


def g(seed, *shape):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(shape).astype(np.float32))


# ------------------------------------------------------------------------------------------------ 1. splat
def golden_splat():
    cases = []
    demo = "/root/reference/assets/results/demo"
    for name in sorted(os.listdir(demo)):
        st = json.load(open(os.path.join(demo, name, "state", "state.json")))
        for idx in (0, -1):
            cases.append((name, st["ellipse_lists"][idx][0], 512, 512, 64, 64))
    cases.append(("move_hat_cli", [[361.1067, 367.8526], [85.4812, 103.6543], 87.3739], 512, 512, 64, 64))
    cases.append(("hires_768", [[541.66, 551.78], [128.22, 155.48], 87.3739], 768, 768, 96, 96))
    cases.append(("nonsquare", [[300.0, 120.0], [60.0, 150.0], 33.0], 640, 384, 48, 80))
    cases.append(("degenerate", [[256.0, 256.0], [1e-5, 1e-5], 0.0], 512, 512, 64, 64))     # app:1384 'add' start ellipse
    out = {}
    meta = []
    for i, (name, ell, W, H, h, w) in enumerate(cases):
        mean, cov = ref_inf.get_gs_from_ellipse(ell)
        nm, nc = ref_inf.normalize_gs(mean, cov, W, H)
        blob = ref_inf.get_blob_dict_from_norm_gs(nm, nc)
        score = splat_features(**blob, score_size=(h, w), return_d_score=True)          # [1,2,h,w] float64
        out[f"score_{i}"] = score.numpy()
        out[f"mean_{i}"] = nm
        out[f"cov_{i}"] = nc
        meta.append(dict(name=name, ellipse=ell, W=W, H=H, h=h, w=w))
    # size < 0.5 branch (ut:165-172)
    blob = ref_inf.get_blob_dict_from_norm_gs(out["mean_0"], out["cov_0"])
    blob["sizes"] = torch.tensor([[0.2]])
    out["score_absent"] = splat_features(**blob, score_size=(64, 64), return_d_score=True).numpy()
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(OUT, "splat.npz"), **out)
    s = out["score_%d" % [m["name"] for m in meta].index("move_hat_cli")]
    print("splat: fg.sum=%.6f fg.max=%.6f" % (s[0, 1].sum(), s[0, 1].max()))


# ------------------------------------------------------------------------------------------------ 1b. blob visualisation
def viz_boost(s):
    """A viz_score_fn that is not the identity: the `s * 1.5` enlargement the reference's docstring names (ut:109), clamped."""
    return s.mul(1.5).clamp(max=1)


def golden_blob_viz():
    """splat_features beyond the pipeline's branch (ut:120-241), splat_features_from_scores (ut:57-77) and pyramid_resize (ut:280-294)
    from the real reference: the app's blob image call (app:637-650), the dictionary return, the stand-alone helpers.  The palette is
    drawn here (numpy PCG64) and stored with the outputs: the reference's own colour table is program text and is not copied."""
    import time
    from blobctrl.utils import utils as ut
    rng = np.random.Generator(np.random.PCG64(2024))
    colors = torch.from_numpy(rng.random((29, 3), dtype=np.float32))
    out, meta = {"viz_colors": colors.numpy()}, {}

    def blob_of(ell, W, H, size=1.0):
        mean, cov = ref_inf.get_gs_from_ellipse(ell)
        nm, nc = ref_inf.normalize_gs(mean, cov, W, H)
        blob = ref_inf.get_blob_dict_from_norm_gs(nm, nc)
        blob["sizes"] = torch.tensor([[size]])
        return blob

    def app_call(blob, viz_size, fn=ut.viz_score_fn):             # app:638-646 keyword for keyword (palette apart)
        return splat_features(**blob, interp_size=64, viz_size=viz_size, is_viz=True, ret_layout=True, score_size=64,
                              viz_score_fn=fn, viz_colors=colors, only_vis=True)["feature_img"]

    # 1. the app's call on small grids
    demo = "/root/reference/assets/results/demo"
    cases = []
    for name in ("move_hat", "enlarge_deer"):                     # two demo states whose first and last ellipse differ
        st = json.load(open(os.path.join(demo, name, "state", "state.json")))
        for idx in (0, -1):
            cases.append(dict(name=f"{name}[{idx}]", ellipse=st["ellipse_lists"][idx][0], W=512, H=512, viz=[40, 40], size=1.0))
    cases.append(dict(name="nonsquare", ellipse=[[300.0, 120.0], [60.0, 150.0], 33.0], W=640, H=384, viz=[48, 80], size=1.0))
    cases.append(dict(name="degenerate", ellipse=[[256.0, 256.0], [1e-5, 1e-5], 0.0], W=512, H=512, viz=[40, 40], size=1.0))   # app:1384
    cases.append(dict(name="absent", ellipse=cases[0]["ellipse"], W=512, H=512, viz=[40, 40], size=0.2))
    for i, c in enumerate(cases):
        img = app_call(blob_of(c["ellipse"], c["W"], c["H"], c["size"]), tuple(c["viz"]))
        assert img.dtype == torch.float64 and tuple(img.shape) == (1, 3) + tuple(c["viz"])
        out[f"app_{i}"] = img.numpy()
    meta["app"] = cases

    # 2. one full-resolution app call as the uint8 image the app makes of it (app:647-648) + its near-integer entries
    full = cases[1]
    blob = blob_of(full["ellipse"], 512, 512)
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        img = app_call(blob, (512, 512))
        hwc = img[0].permute(1, 2, 0).contiguous().cpu().numpy()
        u8 = (hwc * 255).astype(np.uint8)
        times.append(time.perf_counter() - t0)
    v = hwc * 255
    near = np.argwhere(np.abs(v - np.round(v)) < 1e-6)
    assert len(near) <= 1e-4 * hwc.size, f"{len(near)} near-integer entries: take another palette seed"
    out["full_u8"], out["full_near_pos"] = u8, near.astype(np.int32)
    out["full_near_val"] = hwc[tuple(near.T)] if len(near) else np.zeros(0)
    meta["full"] = dict(ellipse=full["ellipse"], W=512, H=512, near=int(len(near)),
                        reference_cpu_ms_median_of_5=1e3 * float(np.median(times)), threads=torch.get_num_threads())

    # 3. dictionary returns
    feats = torch.from_numpy(rng.standard_normal((1, 2, 16)))
    out["dict_features"] = feats.numpy()
    ell = cases[1]["ellipse"]
    meta["dict"] = dict(ellipse=ell, W=512, H=512, ns_ellipse=cases[4]["ellipse"], ns_W=640, ns_H=384)
    d0 = splat_features(**blob_of(ell, 512, 512), score_size=(64, 64), interp_size=16, features=feats)
    d1 = splat_features(**blob_of(cases[4]["ellipse"], 640, 384), score_size=(48, 80), interp_size=20, features=feats, is_viz=True,
                        viz_size=32, viz_colors=colors)
    for tag, d in (("d0", d0), ("d1", d1)):
        assert d["feature_img"] is None and d["entropy_img"] is None
        meta[tag + "_keys"] = sorted(d.keys())
        meta[tag + "_levels"] = sorted(int(k) for k in d["scores_pyramid"])
        for k, lvl in d["scores_pyramid"].items():
            out[f"{tag}_pyr_{int(k)}"] = lvl.numpy()
        for k in ("feature_grid", "raw_scores", "composed_scores"):
            out[f"{tag}_{k}"] = d[k].numpy()
    try:
        splat_features(**blob_of(cases[4]["ellipse"], 640, 384), score_size=(48, 80), interp_size=16, features=feats)
        raise AssertionError("expected KeyError")
    except KeyError:
        meta["keyerror"] = dict(score_size=[48, 80], interp_size=16)

    # 4. int viz_size, fg / bg only, a viz_score_fn that is not the identity
    b = blob_of(ell, 512, 512)
    out["vis_int32"] = splat_features(**b, score_size=(64, 64), viz_size=32, is_viz=True, viz_colors=colors, only_vis=True)["feature_img"].numpy()
    out["fg_only"] = splat_features(**b, score_size=(64, 64), return_d_score=True, only_splatting_fg=True).contiguous().numpy()
    out["bg_only"] = splat_features(**b, score_size=(64, 64), return_d_score=True, only_splatting_bg=True).contiguous().numpy()
    out["app_boost"] = app_call(b, (40, 40), fn=viz_boost).numpy()

    # 5. the helpers stand-alone
    S = rng.random((2, 3, 9, 14))
    Fm = rng.standard_normal((2, 3, 5))
    out["sfs_scores"], out["sfs_features"] = S, Fm
    for dt in ("f64", "f32"):
        tdt = torch.float64 if dt == "f64" else torch.float32
        s_cf, f = torch.from_numpy(S).to(tdt), torch.from_numpy(Fm).to(tdt)
        for cl in (0, 1):
            sc = s_cf.permute(0, 2, 3, 1).contiguous() if cl else s_cf
            for tag, size in (("none", None), ("7", 7), ("9x14", (9, 14))):
                r = ut.splat_features_from_scores(sc, f, size, channels_last=bool(cl))
                assert r.dtype == tdt
                out[f"sfs_{dt}_cl{cl}_{tag}"] = r.numpy()
    P = rng.random((1, 2, 48, 80))
    out["pyr_in"] = P
    pyr = ut.pyramid_resize(torch.from_numpy(P), 20)
    meta["pyr_levels"] = sorted(int(k) for k in pyr)
    for k, lvl in pyr.items():
        if int(k) != 80:
            out[f"pyr_{int(k)}"] = lvl.numpy()
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(OUT, "blob_viz.npz")
    np.savez_compressed(path, **out)
    print("blob_viz: %d arrays, %.1f KB, near-integer entries of the 512^2 image: %d, reference CPU %.1f ms" %
          (len(out), os.path.getsize(path) / 1024, len(near), meta["full"]["reference_cpu_ms_median_of_5"]))


# ------------------------------------------------------------------------------------------------ 2. nets
def golden_nets():
    unet, blob = build_tiny()
    c = TINY
    out = {}
    # "odd": canvas 10 x 24 (latent 10 x 12) - feature maps 10x24 -> 5x12 -> 3x6 -> 2x3: the explicit-size upsampling branch
    for tag, (h, w) in (("wide", (8, 16)), ("square", (8, 8)), ("odd", (10, 24))):
        B = 2
        x_b = g(11, B, 4 + 1 + c["feat"], h, w)
        t = torch.tensor(981)
        down, mid, up = blob(x_b, t, conditioning_scale=0.8, return_dict=False)
        out[f"{tag}_blob_in"] = x_b.numpy()
        for i, r in enumerate(down):
            out[f"{tag}_down_{i}"] = r.numpy()
        out[f"{tag}_mid"] = mid.numpy()
        for i, r in enumerate(up):
            out[f"{tag}_up_{i}"] = r.numpy()
        x_u = g(12, B, 5, h, w)
        ehs = g(13, B, 7, c["ctx"])
        sq = (lambda r: r[..., -r.shape[-2]:])
        eps = unet(x_u, t, encoder_hidden_states=ehs,
                   down_block_add_samples=[sq(r).clone() for r in down], mid_block_add_sample=sq(mid).clone(),
                   up_block_add_samples=[sq(r).clone() for r in up], return_dict=False)[0]
        eps_plain = unet(x_u, t, encoder_hidden_states=ehs, return_dict=False)[0]
        out[f"{tag}_unet_in"] = x_u.numpy()
        out[f"{tag}_ehs"] = ehs.numpy()
        out[f"{tag}_eps"] = eps.numpy()
        out[f"{tag}_eps_plain"] = eps_plain.numpy()
    out["timestep"] = np.array(981)
    np.savez_compressed(os.path.join(OUT, "nets_tiny.npz"), **out)
    print("nets: eps std %.4f, residual-coupled delta %.4f" % (out["wide_eps"].std(),
                                                               np.abs(out["wide_eps"] - out["wide_eps_plain"]).max()))


# ------------------------------------------------------------------------------------------------ 3. schedulers
def golden_schedulers():
    out = {}
    for n in (5, 20, 50):
        uni = UniPCMultistepScheduler(**SD_SCHED)
        ddim = DDIMScheduler(**SD_SCHED, clip_sample=False, set_alpha_to_one=False)
        for name, sch in (("unipc", uni), ("ddim", ddim)):
            sch.set_timesteps(n)
            out[f"{name}_{n}_timesteps"] = sch.timesteps.numpy()
            x = g(21, 1, 4, 8, 8)
            xs = [x.numpy()]
            for i, t in enumerate(sch.timesteps):
                eps = g(100 + i, 1, 4, 8, 8)
                x = sch.step(eps, t, x, return_dict=False)[0]
                xs.append(x.numpy())
            out[f"{name}_{n}_traj"] = np.stack(xs)
        out[f"unipc_{n}_sigmas"] = uni.sigmas.numpy()
    np.savez_compressed(os.path.join(OUT, "schedulers.npz"), **out)
    print("schedulers: unipc50 t0..2", out["unipc_50_timesteps"][:3], "ddim50", out["ddim_50_timesteps"][:3])


def golden_schedulers_eta():
    """Stochastic DDIM (scheduling_ddim.py:342-468 with eta > 0): reference trajectories with an explicit `variance_noise` per step
    (noise_i = g(200 + i)), same inputs as golden_schedulers, plus one run that draws the noise from a CPU generator."""
    out = {}
    for n in (5, 20, 50):
        for eta in (0.3, 1.0):
            sch = DDIMScheduler(**SD_SCHED, clip_sample=False, set_alpha_to_one=False)
            sch.set_timesteps(n)
            x = g(21, 1, 4, 8, 8)
            xs = [x.numpy()]
            for i, t in enumerate(sch.timesteps):
                x = sch.step(g(100 + i, 1, 4, 8, 8), t, x, eta=eta, variance_noise=g(200 + i, 1, 4, 8, 8), return_dict=False)[0]
                xs.append(x.numpy())
            out[f"ddim_{n}_eta{int(round(eta * 10)):02d}_traj"] = np.stack(xs)
    sch = DDIMScheduler(**SD_SCHED, clip_sample=False, set_alpha_to_one=False)
    sch.set_timesteps(5)
    gen = torch.Generator().manual_seed(77)
    x = g(21, 1, 4, 8, 8)
    xs = [x.numpy()]
    for i, t in enumerate(sch.timesteps):
        x = sch.step(g(100 + i, 1, 4, 8, 8), t, x, eta=1.0, generator=gen, return_dict=False)[0]
        xs.append(x.numpy())
    out["ddim_5_eta10_gen77_traj"] = np.stack(xs)
    np.savez_compressed(os.path.join(OUT, "schedulers_eta.npz"), **out)
    print("schedulers_eta:", sorted(out))


class _TapNoise:
    """Records every `randn_tensor` call DDIMScheduler.step (or another scheduler module's step) makes (the variance noise the
    reference drew), in call order."""

    def __init__(self, module="diffusers.schedulers.scheduling_ddim"):
        import importlib
        m = importlib.import_module(module)
        self.m, self.orig, self.drawn = m, m.randn_tensor, []

    def __enter__(self):
        def tapped(*a, **k):
            r = self.orig(*a, **k)
            self.drawn.append(r.detach().clone())
            return r
        self.m.randn_tensor = tapped
        return self

    def __exit__(self, *exc):
        self.m.randn_tensor = self.orig


def golden_loop_eta():
    """golden_loop's body (tiny nets, CFG 7.5, DDIM) with stochastic steps: `sch.step(eps, t, x, eta=, generator=CPU generator)`.
    Stores the final latents, the latents entering every step (teacher-forcing inputs), the guided eps and the noise the reference
    drew; plus `randn_tensor` with a list of three generators (one sample each), for the noise-drawing helper."""
    from diffusers.utils.torch_utils import randn_tensor
    unet, blob = build_tiny()
    c = TINY
    h = w = 8
    B = 1
    out = {}
    pipe = StableDiffusionBlobNetPipeline.__new__(StableDiffusionBlobNetPipeline)
    for steps, (gs, ge), eta, seed in ((5, (0.0, 1.0), 1.0, 1234), (6, (0.0, 0.67), 0.5, 4321)):
        sch = DDIMScheduler(**SD_SCHED, clip_sample=False, set_alpha_to_one=False)
        sch.set_timesteps(steps)
        gen = torch.Generator().manual_seed(seed)
        latents = g(31, B, 4, h, w) * sch.init_noise_sigma
        prompt = g(32, 2 * B, 7, c["ctx"])
        fg_lat = (g(33, 1, 4, h, w) * 0.18215 * 5).repeat(2 * B, 1, 1, 1)
        bg_lat = (g(34, 1, 4, h, w) * 0.18215 * 5).repeat(2 * B, 1, 1, 1)
        ell = [[40.0, 42.0], [20.0, 30.0], 25.0]
        mean, cov = ref_inf.get_gs_from_ellipse(ell)
        nm, nc = ref_inf.normalize_gs(mean, cov, 64, 64)
        gs_score = splat_features(**ref_inf.get_blob_dict_from_norm_gs(nm, nc), score_size=(h, w), return_d_score=True)
        bg_s, fg_s = gs_score.unbind(dim=1)
        bg_s = bg_s.unsqueeze(1).repeat(2 * B, 1, 1, 1).float()
        fg_s = fg_s.unsqueeze(1).repeat(2 * B, 1, 1, 1).float()
        dino = g(35, 1, 1, c["feat"])
        feats = pipe.splat_features_from_scores(fg_s, dino.repeat(2 * B, 1, 1), size=h, channels_last=False)
        keep = [1.0 - float(i / steps < gs or (i + 1) / steps > ge) for i in range(steps)]
        eps_trace, lat_trace = [], []
        with _TapNoise() as tap:
            for i, t in enumerate(sch.timesteps):
                lat_trace.append(latents.numpy().copy())
                lmi = sch.scale_model_input(torch.cat([latents] * 2), t)
                bi = pipe.construct_blobnet_input(lmi, fg_s, fg_lat, feats, background=False)
                d, m, u = blob(bi, t, conditioning_scale=1.0 * keep[i], return_dict=False)
                ui = pipe.construct_blobnet_input(lmi, bg_s, bg_lat, background=True)
                npred = unet(ui, t, encoder_hidden_states=prompt, down_block_add_samples=[x[..., -x.shape[-2]:] for x in d],
                             mid_block_add_sample=m[..., -m.shape[-2]:], up_block_add_samples=[x[..., -x.shape[-2]:] for x in u],
                             return_dict=False)[0]
                b_, c_, h_, w_ = npred.shape
                npred = npred[..., :h_, w_ // 2:]
                nu, nt = npred.chunk(2)
                npred = nu + 7.5 * (nt - nu)
                eps_trace.append(npred.numpy())
                latents = sch.step(npred, t, latents, eta=eta, generator=gen, return_dict=False)[0]
        assert len(tap.drawn) == steps
        tag = f"ddim_{steps}"
        out[f"{tag}_final"] = latents.numpy()
        out[f"{tag}_eps"] = np.stack(eps_trace)
        out[f"{tag}_lat"] = np.stack(lat_trace)
        out[f"{tag}_noise"] = torch.stack(tap.drawn).numpy()
        out[f"{tag}_window"] = np.array([gs, ge])
        out[f"{tag}_eta"] = np.array(eta)
        out[f"{tag}_seed"] = np.array(seed)
        print(f"loop_eta {tag}: eta {eta}, final std {latents.std():.4f}")
    gens = [torch.Generator().manual_seed(s_) for s_ in (11, 12, 13)]
    out["list3_seeds"] = np.array([11, 12, 13])
    out["list3_noise"] = torch.stack([randn_tensor((3, 4, h, w), generator=gens, device=torch.device("cpu"), dtype=torch.float32)
                                      for _ in range(2)]).numpy()
    np.savez_compressed(os.path.join(OUT, "loop_tiny_eta.npz"), **out)


# DPM-Solver cases of schedulers_dpm.npz: name -> (DPMSolverMultistepScheduler options on top of SD_SCHED, steps, caller timesteps)
DPM_CUSTOM_TS = [999, 850, 736, 645, 545, 455, 343, 233, 124, 24]
DPM_CASES = {
    "pp2_mid_lin_5": (dict(), 5, None),
    "pp2_mid_lin_14": (dict(), 14, None),
    "pp2_mid_lin_15": (dict(), 15, None),
    "pp2_heun_lin_20": (dict(solver_type="heun"), 20, None),
    "pp2_mid_karras_50": (dict(use_karras_sigmas=True), 50, None),
    "pp2_heun_karras_14": (dict(use_karras_sigmas=True, solver_type="heun"), 14, None),
    "pp2_mid_lu_5": (dict(use_lu_lambdas=True), 5, None),
    "pp2_mid_leading_5": (dict(timestep_spacing="leading"), 5, None),
    "pp2_mid_trailing_5": (dict(timestep_spacing="trailing"), 5, None),
    "pp2_sigmamin_15": (dict(final_sigmas_type="sigma_min"), 15, None),
    "pp2_sigmamin_euler_15": (dict(final_sigmas_type="sigma_min", euler_at_final=True), 15, None),
    "pp2_sigmamin_5": (dict(final_sigmas_type="sigma_min"), 5, None),
    "pp1_lin_5": (dict(solver_order=1), 5, None),
    "pp3_lin_5": (dict(solver_order=3), 5, None),
    "pp3_lin_14": (dict(solver_order=3), 14, None),
    "pp3_karras_15": (dict(solver_order=3, use_karras_sigmas=True), 15, None),
    "pp3_lu_sigmamin_5": (dict(solver_order=3, use_lu_lambdas=True, final_sigmas_type="sigma_min"), 5, None),
    "pp2_custom_10": (dict(), None, DPM_CUSTOM_TS),
    "pp3_custom_10": (dict(solver_order=3), None, DPM_CUSTOM_TS),
    "sde1_lin_5": (dict(algorithm_type="sde-dpmsolver++", solver_order=1), 5, None),
    "sde2_mid_lin_15": (dict(algorithm_type="sde-dpmsolver++"), 15, None),
    "sde2_heun_karras_14": (dict(algorithm_type="sde-dpmsolver++", solver_type="heun", use_karras_sigmas=True), 14, None),
    "sde2_mid_lu_5": (dict(algorithm_type="sde-dpmsolver++", use_lu_lambdas=True), 5, None),
    "sde2_trailing_sigmamin_5": (dict(algorithm_type="sde-dpmsolver++", timestep_spacing="trailing", final_sigmas_type="sigma_min"),
                                 5, None),
    "sde2_custom_10": (dict(algorithm_type="sde-dpmsolver++"), None, DPM_CUSTOM_TS),
}
SD15_SCHEDULER_JSON = {"_class_name": "PNDMScheduler", "_diffusers_version": "0.6.0", "beta_end": 0.012, "beta_schedule": "scaled_linear",
                       "beta_start": 0.00085, "num_train_timesteps": 1000, "set_alpha_to_one": False, "skip_prk_steps": True,
                       "steps_offset": 1, "trained_betas": None, "clip_sample": False}


def golden_schedulers_dpm():
    """DPMSolverMultistepScheduler (scheduling_dpmsolver_multistep.py) on golden_schedulers' inputs (8x8 latents, eps_i = g(100 + i)),
    the SDE noise given as variance_noise = g(200 + i): timesteps, sigmas and trajectories of DPM_CASES, plus one SDE run that draws
    from a CPU generator.  The `.config` of `from_config(<SD-1.5 scheduler_config.json>)` goes to dpm_config.json."""
    from diffusers import DPMSolverMultistepScheduler, PNDMScheduler
    out = {}
    for name, (kw, n, ts) in DPM_CASES.items():
        sch = DPMSolverMultistepScheduler(**SD_SCHED, **kw)
        if ts is not None:
            sch.set_timesteps(timesteps=ts)
        else:
            sch.set_timesteps(n)
        sde = kw.get("algorithm_type") == "sde-dpmsolver++"
        x = g(21, 1, 4, 8, 8)
        xs = [x.numpy()]
        for i, t in enumerate(sch.timesteps):
            x = sch.step(g(100 + i, 1, 4, 8, 8), t, x, variance_noise=g(200 + i, 1, 4, 8, 8) if sde else None, return_dict=False)[0]
            xs.append(x.numpy())
        out[f"{name}_timesteps"] = sch.timesteps.numpy()
        out[f"{name}_sigmas"] = sch.sigmas.numpy()
        out[f"{name}_traj"] = np.stack(xs)
        out[f"{name}_kw"] = np.array(json.dumps(dict(kw, timesteps=ts, n=n)))
    sch = DPMSolverMultistepScheduler(**SD_SCHED, algorithm_type="sde-dpmsolver++")
    sch.set_timesteps(5)
    gen = torch.Generator().manual_seed(77)
    x = g(21, 1, 4, 8, 8)
    xs = [x.numpy()]
    for i, t in enumerate(sch.timesteps):
        x = sch.step(g(100 + i, 1, 4, 8, 8), t, x, generator=gen, return_dict=False)[0]
        xs.append(x.numpy())
    out["sde2_gen77_5_traj"] = np.stack(xs)
    np.savez_compressed(os.path.join(OUT, "schedulers_dpm.npz"), **out)
    cfg = dict(DPMSolverMultistepScheduler.from_config(SD15_SCHEDULER_JSON).config)
    via_pndm = dict(DPMSolverMultistepScheduler.from_config(PNDMScheduler.from_config(SD15_SCHEDULER_JSON).config).config)
    for c in (cfg, via_pndm):
        c["_use_default_values"] = sorted(c["_use_default_values"])
    assert cfg == via_pndm, (cfg, via_pndm)
    with open(os.path.join(OUT, "dpm_config.json"), "w") as f:
        json.dump({"source": SD15_SCHEDULER_JSON, "config": cfg}, f, indent=1, sort_keys=True)
    print("schedulers_dpm:", len(DPM_CASES), "cases; config keys", sorted(cfg))


# DPM-Solver cases of loop_tiny_dpm.npz: tag -> (options on top of SD_SCHED, steps, caller timesteps, guidance window, generator seed)
DPM_LOOPS = {
    "karras2m_6": (dict(use_karras_sigmas=True), 6, None, (0.0, 0.67), None),
    "sde2m_5": (dict(algorithm_type="sde-dpmsolver++"), 5, None, (0.0, 1.0), 1234),
    "dpm3m_6": (dict(solver_order=3), 6, None, (0.0, 1.0), None),
    "custom2m_10": (dict(), None, DPM_CUSTOM_TS, (0.0, 0.9), None),
}


def golden_loop_dpm():
    """golden_loop's body (tiny nets, CFG 7.5) with DPM-Solver++: 2M Karras, SDE 2M (CPU generator, noise tapped from step), 3M, and
    2M on caller timesteps.  Stores the final latents, the latents entering every step and the guided eps."""
    from diffusers import DPMSolverMultistepScheduler
    unet, blob = build_tiny()
    c = TINY
    h = w = 8
    B = 1
    out = {}
    pipe = StableDiffusionBlobNetPipeline.__new__(StableDiffusionBlobNetPipeline)
    for tag, (kw, steps, ts, (gs, ge), seed) in DPM_LOOPS.items():
        sch = DPMSolverMultistepScheduler(**SD_SCHED, **kw)
        if ts is not None:
            sch.set_timesteps(timesteps=ts)
        else:
            sch.set_timesteps(steps)
        steps = len(sch.timesteps)
        gen = torch.Generator().manual_seed(seed) if seed is not None else None
        latents = g(31, B, 4, h, w) * sch.init_noise_sigma
        prompt = g(32, 2 * B, 7, c["ctx"])
        fg_lat = (g(33, 1, 4, h, w) * 0.18215 * 5).repeat(2 * B, 1, 1, 1)
        bg_lat = (g(34, 1, 4, h, w) * 0.18215 * 5).repeat(2 * B, 1, 1, 1)
        ell = [[40.0, 42.0], [20.0, 30.0], 25.0]
        mean, cov = ref_inf.get_gs_from_ellipse(ell)
        nm, nc = ref_inf.normalize_gs(mean, cov, 64, 64)
        gs_score = splat_features(**ref_inf.get_blob_dict_from_norm_gs(nm, nc), score_size=(h, w), return_d_score=True)
        bg_s, fg_s = gs_score.unbind(dim=1)
        bg_s = bg_s.unsqueeze(1).repeat(2 * B, 1, 1, 1).float()
        fg_s = fg_s.unsqueeze(1).repeat(2 * B, 1, 1, 1).float()
        dino = g(35, 1, 1, c["feat"])
        feats = pipe.splat_features_from_scores(fg_s, dino.repeat(2 * B, 1, 1), size=h, channels_last=False)
        keep = [1.0 - float(i / steps < gs or (i + 1) / steps > ge) for i in range(steps)]
        eps_trace, lat_trace = [], []
        with _TapNoise("diffusers.schedulers.scheduling_dpmsolver_multistep") as tap:
            for i, t in enumerate(sch.timesteps):
                lat_trace.append(latents.numpy().copy())
                lmi = sch.scale_model_input(torch.cat([latents] * 2), t)
                bi = pipe.construct_blobnet_input(lmi, fg_s, fg_lat, feats, background=False)
                d, m, u = blob(bi, t, conditioning_scale=1.0 * keep[i], return_dict=False)
                ui = pipe.construct_blobnet_input(lmi, bg_s, bg_lat, background=True)
                npred = unet(ui, t, encoder_hidden_states=prompt, down_block_add_samples=[x[..., -x.shape[-2]:] for x in d],
                             mid_block_add_sample=m[..., -m.shape[-2]:], up_block_add_samples=[x[..., -x.shape[-2]:] for x in u],
                             return_dict=False)[0]
                b_, c_, h_, w_ = npred.shape
                npred = npred[..., :h_, w_ // 2:]
                nu, nt = npred.chunk(2)
                npred = nu + 7.5 * (nt - nu)
                eps_trace.append(npred.numpy())
                latents = sch.step(npred, t, latents, generator=gen, return_dict=False)[0]
        assert len(tap.drawn) == (steps if seed is not None else 0)
        out[f"{tag}_final"] = latents.numpy()
        out[f"{tag}_eps"] = np.stack(eps_trace)
        out[f"{tag}_lat"] = np.stack(lat_trace)
        out[f"{tag}_timesteps"] = sch.timesteps.numpy()
        out[f"{tag}_window"] = np.array([gs, ge])
        out[f"{tag}_kw"] = np.array(json.dumps(dict(kw, timesteps=ts, n=steps)))
        if seed is not None:
            out[f"{tag}_noise"] = torch.stack(tap.drawn).numpy()
            out[f"{tag}_seed"] = np.array(seed)
        print(f"loop_dpm {tag}: {steps} steps, final std {latents.std():.4f}")
    np.savez_compressed(os.path.join(OUT, "loop_tiny_dpm.npz"), **out)


def golden_pipeline_call_dpm():
    """The reference's own `__call__` (pipe:743-1166) with an SDE-DPM-Solver++ 2M scheduler, caller `timesteps` (retrieve_timesteps,
    pipe:114-155) and a CPU `generator` (start latents, then every step's noise: pipe:313-328, 1102).  Case = `ddim_neg2` of
    pipeline_call.npz with its own seeds; the images and scores are those of pipeline_call.npz."""
    from PIL import Image
    from diffusers import DPMSolverMultistepScheduler
    from tests.common import FakeTokenizer, pipeline_cases
    unet, blob, vae, te, proc, dino = _tiny_pipeline_components()
    base = np.load(os.path.join(OUT, "pipeline_call.npz"))
    kw = dict(pipeline_cases()["ddim_neg2"], seed=2025, rng_seed=22)
    kw.pop("scheduler"), kw.pop("num_inference_steps")
    timesteps = [999, 750, 500, 250]
    sch = DPMSolverMultistepScheduler.from_config(DDIMScheduler(**SD_SCHED, clip_sample=False, set_alpha_to_one=False).config,
                                                  algorithm_type="sde-dpmsolver++")
    pipe = StableDiffusionBlobNetPipeline(vae=vae, unet=unet, tokenizer=FakeTokenizer(), text_encoder=te, blobnet=blob, scheduler=sch,
                                          safety_checker=None, dinov2_processor=proc, dinov2=dino, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    seed, rng_seed = kw.pop("seed"), kw.pop("rng_seed")
    out = {"seed": np.array(seed), "rng_seed": np.array(rng_seed), "timesteps": np.array(timesteps)}
    torch.manual_seed(rng_seed)
    with _TapNoise("diffusers.schedulers.scheduling_dpmsolver_multistep") as noise:
        r = pipe(fg_image=Image.fromarray(base["fg"]), bg_image=Image.fromarray(base["bg"]), gs_score=torch.from_numpy(base["gs_score"]),
                 height=64, width=64, timesteps=timesteps, generator=torch.Generator().manual_seed(seed), output_type="latent", **kw)
    assert len(noise.drawn) == len(timesteps) and pipe.num_timesteps == len(timesteps)
    out["latents"] = r.images.numpy()
    out["noise"] = torch.stack(noise.drawn).numpy()
    out["scheduler_timesteps"] = sch.timesteps.numpy()
    np.savez_compressed(os.path.join(OUT, "pipeline_call_dpm.npz"), **out)
    print(f"pipeline __call__ sde-dpm++ 2m on {timesteps}: latents std {out['latents'].std():.4f}, noise {out['noise'].shape}")


# ------------------------------------------------------------------------------------------------ Euler / Euler-ancestral / Heun
class _GiveNoise:
    """Makes every `randn_tensor` call of a scheduler module return the next tensor of `noises` (EulerAncestralDiscreteScheduler.step has
    no variance_noise argument: this is how a trajectory with GIVEN noise is run through the reference)."""

    def __init__(self, module, noises):
        import importlib
        m = importlib.import_module(module)
        self.m, self.orig, self.noises = m, m.randn_tensor, list(noises)

    def __enter__(self):
        self.m.randn_tensor = lambda *a, **k: self.noises.pop(0)
        return self

    def __exit__(self, *exc):
        self.m.randn_tensor = self.orig


EULER_A_MODULE = "diffusers.schedulers.scheduling_euler_ancestral_discrete"
EULER_CUSTOM_TS = [999, 850, 736, 645, 545, 455, 343, 233, 124, 24]
# cases of schedulers_euler.npz: name -> (scheduler class key, options on top of SD_SCHED, steps, caller timesteps)
EULER_CASES = {
    "euler_leading_5": ("euler", dict(timestep_spacing="leading"), 5, None),
    "euler_leading_20": ("euler", dict(timestep_spacing="leading"), 20, None),
    "euler_leading_50": ("euler", dict(timestep_spacing="leading"), 50, None),
    "euler_linspace_15": ("euler", dict(), 15, None),
    "euler_trailing_karras_10": ("euler", dict(timestep_spacing="trailing", use_karras_sigmas=True), 10, None),
    "euler_sigmamin_8": ("euler", dict(final_sigmas_type="sigma_min"), 8, None),
    "euler_custom_10": ("euler", dict(), None, EULER_CUSTOM_TS),
    "eulera_noise_15": ("euler_ancestral", dict(), 15, None),
    "eulera_leading_noise_5": ("euler_ancestral", dict(timestep_spacing="leading"), 5, None),
    "heun_10": ("heun", dict(), 10, None),
    "heun_karras_6": ("heun", dict(use_karras_sigmas=True), 6, None),
    "heun_leading_5": ("heun", dict(timestep_spacing="leading"), 5, None),
}


def _euler_class(key):
    from diffusers import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler, HeunDiscreteScheduler
    return {"euler": EulerDiscreteScheduler, "euler_ancestral": EulerAncestralDiscreteScheduler, "heun": HeunDiscreteScheduler}[key]


def golden_schedulers_euler():
    """EulerDiscreteScheduler, EulerAncestralDiscreteScheduler and HeunDiscreteScheduler on golden_schedulers' inputs (8x8 latents
    x = g(21) * init_noise_sigma, eps_i = g(100 + i)), the ancestral noise GIVEN as g(200 + i): timesteps, sigmas, init_noise_sigma, the
    per-step scale_model_input of the fixed tensor g(22) and the trajectories of EULER_CASES, plus one ancestral run that draws from a
    CPU generator.  The `.config` of `from_config(<SD-1.5 scheduler_config.json>)` of the three classes goes to euler_config.json."""
    from diffusers import PNDMScheduler
    out = {}

    def run(sch, n, ts, step_kw):
        sch.set_timesteps(timesteps=ts) if ts is not None else sch.set_timesteps(n)
        fixed = g(22, 1, 4, 8, 8)
        x = g(21, 1, 4, 8, 8) * sch.init_noise_sigma
        xs, scaled = [x.numpy()], []
        for i, t in enumerate(sch.timesteps):
            scaled.append(sch.scale_model_input(fixed, t).numpy())
            x = sch.step(g(100 + i, 1, 4, 8, 8), t, x, return_dict=False, **step_kw)[0]
            xs.append(x.numpy())
        return np.stack(xs), np.stack(scaled)

    for name, (cls, kw, n, ts) in EULER_CASES.items():
        sch = _euler_class(cls)(**SD_SCHED, **kw)
        with _GiveNoise(EULER_A_MODULE, [g(200 + i, 1, 4, 8, 8) for i in range(200)]):
            traj, scaled = run(sch, n, ts, {})
        out[f"{name}_timesteps"] = sch.timesteps.numpy()
        out[f"{name}_sigmas"] = sch.sigmas.numpy()
        out[f"{name}_init_noise_sigma"] = np.array(float(sch.init_noise_sigma))
        out[f"{name}_scaled"] = scaled
        out[f"{name}_traj"] = traj
        out[f"{name}_kw"] = np.array(json.dumps(dict(kw, cls=cls, timesteps=ts, n=n)))
        assert sch.sigmas.dtype == torch.float32, name               # (timesteps: float32, float64 for Heun with Karras sigmas)
    sch = _euler_class("euler_ancestral")(**SD_SCHED)                 # the generator case: the same set of arrays (it has no `_kw` entry:
    name = "eulera_gen77_5"                                           # its noise is not the g(200 + i) of the cases above)
    out[f"{name}_traj"], out[f"{name}_scaled"] = run(sch, 5, None, dict(generator=torch.Generator().manual_seed(77)))
    out[f"{name}_timesteps"] = sch.timesteps.numpy()
    out[f"{name}_sigmas"] = sch.sigmas.numpy()
    out[f"{name}_init_noise_sigma"] = np.array(float(sch.init_noise_sigma))
    # the float32 log-sigmas the Karras timesteps above were interpolated in (scheduling_euler_discrete.py:383-384), as THIS machine's numpy
    # computes them: numpy's float32 log differs in the last bit between CPUs, and with it the fractional Karras timesteps
    ac = sch.alphas_cumprod
    out["train_log_sigmas"] = np.log(np.array(((1 - ac) / ac) ** 0.5))
    np.savez_compressed(os.path.join(OUT, "schedulers_euler.npz"), **out)
    cfgs = {}
    for cls in ("euler", "euler_ancestral", "heun"):
        C = _euler_class(cls)
        cfg = dict(C.from_config(SD15_SCHEDULER_JSON).config)
        via_pndm = dict(C.from_config(PNDMScheduler.from_config(SD15_SCHEDULER_JSON).config).config)
        for c in (cfg, via_pndm):
            c["_use_default_values"] = sorted(c["_use_default_values"])
        assert cfg == via_pndm, (cfg, via_pndm)
        cfgs[cls] = cfg
    with open(os.path.join(OUT, "euler_config.json"), "w") as f:
        json.dump(dict(cfgs, source=SD15_SCHEDULER_JSON), f, indent=1, sort_keys=True)
    print("schedulers_euler:", len(EULER_CASES), "cases; euler config keys", sorted(cfgs["euler"]))


# cases of loop_tiny_euler.npz: tag -> (class key, options on top of SD_SCHED, steps, caller timesteps, guidance window, generator seed)
EULER_LOOPS = {
    "euler_leading_6": ("euler", dict(timestep_spacing="leading"), 6, None, (0.0, 1.0), None),
    "euler_linspace_5": ("euler", dict(), 5, None, (0.0, 1.0), None),
    "euler_karras_6": ("euler", dict(use_karras_sigmas=True), 6, None, (0.0, 0.67), None),
    "eulera_5": ("euler_ancestral", dict(), 5, None, (0.0, 1.0), 1234),
    "heun_4": ("heun", dict(), 4, None, (0.0, 1.0), None),
    "euler_custom_8": ("euler", dict(), None, [999, 850, 700, 550, 400, 250, 120, 20], (0.0, 0.9), None),
}


def golden_loop_euler(dtype=torch.float32, save=True):
    """golden_loop's body (tiny nets, CFG 7.5) with the sigma-space schedulers: the latents start at g(31) * init_noise_sigma, every
    step's model input goes through scheduler.scale_model_input (pipe:1032).  Euler (leading, linspace = fractional timesteps, Karras,
    caller timesteps), Euler-ancestral (CPU generator, noise tapped from step) and Heun (2n - 1 evaluations).  Stores the final latents,
    the latents entering every step and the guided eps.  `dtype=torch.float64, save=False` returns the same loop in float64 (the
    reference's own fp32-versus-fp64 spread)."""
    unet, blob = build_tiny()
    unet, blob = unet.to(dtype), blob.to(dtype)
    c = TINY
    h = w = 8
    B = 1
    out = {}
    pipe = StableDiffusionBlobNetPipeline.__new__(StableDiffusionBlobNetPipeline)
    for tag, (cls, kw, steps, ts, (gs, ge), seed) in EULER_LOOPS.items():
        sch = _euler_class(cls)(**SD_SCHED, **kw)
        if ts is not None:
            sch.set_timesteps(timesteps=ts)
        else:
            sch.set_timesteps(steps)
        evals = len(sch.timesteps)
        gen = torch.Generator().manual_seed(seed) if seed is not None else None
        latents = (g(31, B, 4, h, w) * sch.init_noise_sigma).to(dtype)
        prompt = g(32, 2 * B, 7, c["ctx"]).to(dtype)
        fg_lat = (g(33, 1, 4, h, w) * 0.18215 * 5).repeat(2 * B, 1, 1, 1).to(dtype)
        bg_lat = (g(34, 1, 4, h, w) * 0.18215 * 5).repeat(2 * B, 1, 1, 1).to(dtype)
        ell = [[40.0, 42.0], [20.0, 30.0], 25.0]
        mean, cov = ref_inf.get_gs_from_ellipse(ell)
        nm, nc = ref_inf.normalize_gs(mean, cov, 64, 64)
        gs_score = splat_features(**ref_inf.get_blob_dict_from_norm_gs(nm, nc), score_size=(h, w), return_d_score=True)
        bg_s, fg_s = gs_score.unbind(dim=1)
        bg_s = bg_s.unsqueeze(1).repeat(2 * B, 1, 1, 1).to(dtype)
        fg_s = fg_s.unsqueeze(1).repeat(2 * B, 1, 1, 1).to(dtype)
        dino = g(35, 1, 1, c["feat"]).to(dtype)
        feats = pipe.splat_features_from_scores(fg_s, dino.repeat(2 * B, 1, 1), size=h, channels_last=False)
        keep = [1.0 - float(i / evals < gs or (i + 1) / evals > ge) for i in range(evals)]          # pipe:1006-1012: over len(timesteps)
        eps_trace, lat_trace = [], []
        with _TapNoise(EULER_A_MODULE) as tap:
            for i, t in enumerate(sch.timesteps):
                lat_trace.append(latents.numpy().copy())
                lmi = sch.scale_model_input(torch.cat([latents] * 2), t)
                bi = pipe.construct_blobnet_input(lmi, fg_s, fg_lat, feats, background=False)
                d, m, u = blob(bi, t, conditioning_scale=1.0 * keep[i], return_dict=False)
                ui = pipe.construct_blobnet_input(lmi, bg_s, bg_lat, background=True)
                npred = unet(ui, t, encoder_hidden_states=prompt, down_block_add_samples=[x[..., -x.shape[-2]:] for x in d],
                             mid_block_add_sample=m[..., -m.shape[-2]:], up_block_add_samples=[x[..., -x.shape[-2]:] for x in u],
                             return_dict=False)[0]
                b_, c_, h_, w_ = npred.shape
                npred = npred[..., :h_, w_ // 2:]
                nu, nt = npred.chunk(2)
                npred = nu + 7.5 * (nt - nu)
                eps_trace.append(npred.numpy())
                step_kw = dict(generator=gen) if cls == "euler_ancestral" else {}
                latents = sch.step(npred, t, latents, return_dict=False, **step_kw)[0].to(dtype)
        assert len(tap.drawn) == (evals if seed is not None else 0)
        out[f"{tag}_final"] = latents.numpy()
        out[f"{tag}_eps"] = np.stack(eps_trace)
        out[f"{tag}_lat"] = np.stack(lat_trace)
        out[f"{tag}_timesteps"] = sch.timesteps.numpy()
        out[f"{tag}_window"] = np.array([gs, ge])
        out[f"{tag}_kw"] = np.array(json.dumps(dict(kw, cls=cls, timesteps=ts, n=steps)))
        if seed is not None:
            out[f"{tag}_noise"] = torch.stack(tap.drawn).numpy()
            out[f"{tag}_seed"] = np.array(seed)
        print(f"loop_euler {tag} ({dtype}): {evals} evaluations, final std {latents.std():.4f}")
    if save:
        np.savez_compressed(os.path.join(OUT, "loop_tiny_euler.npz"), **out)
    return out


def euler_loop_spread():
    """The reference's own fp32-versus-fp64 spread of golden_loop_euler's final latents (max-abs / scale), printed per case."""
    a, b = golden_loop_euler(save=False), golden_loop_euler(torch.float64, save=False)
    for tag in EULER_LOOPS:
        x, y = a[f"{tag}_final"].astype(np.float64), b[f"{tag}_final"].astype(np.float64)
        print(f"{tag}: reference fp32 vs fp64 final latents max-abs/scale {np.abs(x - y).max() / np.abs(y).max():.3e}")


def golden_pipeline_call_euler():
    """The reference's own `__call__` (pipe:743-1166) with `EulerDiscreteScheduler.from_config(pipeline.scheduler.config)` (linspace:
    fractional timesteps) and with EulerAncestralDiscreteScheduler (leading spacing) and a CPU `generator` (start latents, then every step's
    noise).  Case = `ddim_neg2` of pipeline_call.npz with its own seeds; the images and scores are those of pipeline_call.npz."""
    from PIL import Image
    from diffusers import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler
    from tests.common import FakeTokenizer, pipeline_cases
    unet, blob, vae, te, proc, dino = _tiny_pipeline_components()
    base = np.load(os.path.join(OUT, "pipeline_call.npz"))
    kw = dict(pipeline_cases()["ddim_neg2"], seed=2026, rng_seed=23)
    kw.pop("scheduler")
    seed, rng_seed = kw.pop("seed"), kw.pop("rng_seed")
    kw["num_inference_steps"] = 5
    src = DDIMScheduler(**SD_SCHED, clip_sample=False, set_alpha_to_one=False)
    pipe = StableDiffusionBlobNetPipeline(vae=vae, unet=unet, tokenizer=FakeTokenizer(), text_encoder=te, blobnet=blob, scheduler=src,
                                          safety_checker=None, dinov2_processor=proc, dinov2=dino, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    out = {"seed": np.array(seed), "rng_seed": np.array(rng_seed), "num_inference_steps": np.array(kw["num_inference_steps"])}
    call = lambda: pipe(fg_image=Image.fromarray(base["fg"]), bg_image=Image.fromarray(base["bg"]), gs_score=torch.from_numpy(base["gs_score"]),
                        height=64, width=64, generator=torch.Generator().manual_seed(seed), output_type="latent", **kw)
    pipe.scheduler = EulerDiscreteScheduler.from_config(src.config)
    torch.manual_seed(rng_seed)
    out["euler_latents"] = call().images.numpy()
    out["euler_timesteps"] = pipe.scheduler.timesteps.numpy()
    pipe.scheduler = EulerAncestralDiscreteScheduler.from_config(src.config, timestep_spacing="leading")
    torch.manual_seed(rng_seed)
    with _TapNoise(EULER_A_MODULE) as noise:
        out["eulera_latents"] = call().images.numpy()
    assert len(noise.drawn) == kw["num_inference_steps"]
    out["eulera_noise"] = torch.stack(noise.drawn).numpy()
    out["eulera_timesteps"] = pipe.scheduler.timesteps.numpy()
    np.savez_compressed(os.path.join(OUT, "pipeline_call_euler.npz"), **out)
    print(f"pipeline __call__ euler {out['euler_timesteps']}: latents std {out['euler_latents'].std():.4f}; euler a "
          f"{out['eulera_timesteps']}: std {out['eulera_latents'].std():.4f}, noise {out['eulera_noise'].shape}")


# ------------------------------------------------------------------------------------------------ LCM (few-step latent-consistency edits)
LCM_MODULE = "diffusers.schedulers.scheduling_lcm"
LCM_CUSTOM_TS = [939, 601, 320, 19]
# cases of schedulers_lcm.npz: name -> (LCMScheduler options on top of SD_SCHED, set_timesteps keyword arguments)
LCM_CASES = {
    "lcm_1": (dict(), dict(num_inference_steps=1)),
    "lcm_2": (dict(), dict(num_inference_steps=2)),
    "lcm_4": (dict(), dict(num_inference_steps=4)),
    "lcm_8": (dict(), dict(num_inference_steps=8)),
    "lcm_50": (dict(), dict(num_inference_steps=50)),
    "lcm_orig30_6": (dict(original_inference_steps=30), dict(num_inference_steps=6)),
    "lcm_orig30_arg_6": (dict(), dict(num_inference_steps=6, original_inference_steps=30)),
    "lcm_scaling5_4": (dict(timestep_scaling=5.0), dict(num_inference_steps=4)),
    "lcm_custom_4": (dict(), dict(timesteps=LCM_CUSTOM_TS)),
    "lcm_strength_3": (dict(), dict(num_inference_steps=3, strength=0.5)),
    # caller timesteps cut by strength: the class keeps num_inference_steps = 4, so the last of the two steps draws noise as well
    "lcm_custom_strength_2": (dict(), dict(timesteps=LCM_CUSTOM_TS, strength=0.5)),
}


def golden_schedulers_lcm():
    """LCMScheduler (scheduling_lcm.py) on golden_schedulers' inputs (8x8 latents x = g(21), eps_i = g(100 + i)), the noise GIVEN as
    g(200 + i): timesteps, the trajectories and the `denoised` outputs of LCM_CASES, the number of noise tensors each run asked for, plus
    one run that draws from a CPU generator.  The `.config` of `from_config(<SD-1.5 scheduler_config.json>)` goes to lcm_config.json."""
    from diffusers import LCMScheduler, PNDMScheduler
    out = {}

    def run(sch, set_kw, step_kw):
        sch.set_timesteps(**set_kw)
        x = g(21, 1, 4, 8, 8) * sch.init_noise_sigma
        xs, den = [x.numpy()], []
        for i, t in enumerate(sch.timesteps):
            x, d = sch.step(g(100 + i, 1, 4, 8, 8), t, x, return_dict=False, **step_kw)
            xs.append(x.numpy())
            den.append(d.numpy())
        return np.stack(xs), np.stack(den)

    for name, (kw, set_kw) in LCM_CASES.items():
        sch = LCMScheduler(**SD_SCHED, set_alpha_to_one=False, **kw)
        noises = [g(200 + i, 1, 4, 8, 8) for i in range(200)]
        with _GiveNoise(LCM_MODULE, noises) as give:
            out[f"{name}_traj"], out[f"{name}_denoised"] = run(sch, set_kw, {})
        out[f"{name}_timesteps"] = sch.timesteps.numpy()
        out[f"{name}_draws"] = np.array(200 - len(give.noises))
        out[f"{name}_kw"] = np.array(json.dumps(dict(options=kw, set_timesteps=set_kw)))
        assert int(out[f"{name}_draws"]) == len(sch.timesteps) - (0 if name == "lcm_custom_strength_2" else 1), name
    sch = LCMScheduler(**SD_SCHED, set_alpha_to_one=False)
    with _TapNoise(LCM_MODULE) as tap:
        out["lcm_gen77_4_traj"], out["lcm_gen77_4_denoised"] = run(sch, dict(num_inference_steps=4),
                                                                   dict(generator=torch.Generator().manual_seed(77)))
    out["lcm_gen77_4_timesteps"] = sch.timesteps.numpy()
    out["lcm_gen77_4_noise"] = torch.stack(tap.drawn).numpy()
    assert len(tap.drawn) == 3
    np.savez_compressed(os.path.join(OUT, "schedulers_lcm.npz"), **out)
    cfg = dict(LCMScheduler.from_config(SD15_SCHEDULER_JSON).config)
    via_pndm = dict(LCMScheduler.from_config(PNDMScheduler.from_config(SD15_SCHEDULER_JSON).config).config)
    via_ddim = dict(LCMScheduler.from_config(DDIMScheduler.from_config(SD15_SCHEDULER_JSON).config).config)
    for c in (cfg, via_pndm, via_ddim):
        c["_use_default_values"] = sorted(c["_use_default_values"])
    assert cfg == via_pndm, (cfg, via_pndm)
    for k in ("original_inference_steps", "timestep_scaling", "timestep_spacing", "steps_offset", "set_alpha_to_one", "clip_sample"):
        assert cfg[k] == via_ddim[k], k
    with open(os.path.join(OUT, "lcm_config.json"), "w") as f:
        json.dump(dict(lcm=cfg, source=SD15_SCHEDULER_JSON), f, indent=1, sort_keys=True)
    print("schedulers_lcm:", len(LCM_CASES), "cases; config", cfg)


# cases of loop_tiny_lcm.npz: tag -> (scheduler class key, set_timesteps keyword arguments, guidance scale, BlobNet window, generator seed)
LCM_LOOPS = {
    "lcm_cfg_4": ("lcm", dict(num_inference_steps=4), 7.5, (0.0, 1.0), 1234),
    "lcm_nocfg_4": ("lcm", dict(num_inference_steps=4), 1.0, (0.0, 0.5), 1234),
    "ddim_single_5": ("ddim", dict(num_inference_steps=5), 1.0, (0.0, 1.0), None),
    "unipc_single_5": ("unipc", dict(num_inference_steps=5), 1.0, (0.0, 0.6), None),
    # the UNet of a distilled LCM model (time_cond_proj_dim = 8): guidance 7.5 goes in as timestep_cond, no CFG (pipe:497)
    "lcm_wcond_4": ("lcm", dict(num_inference_steps=4), 7.5, (0.0, 0.5), 1234),
    "lcm_wcond_custom_3": ("lcm", dict(timesteps=[939, 601, 19]), 3.0, (0.0, 1.0), 4321),
}
LCM_WCOND_DIM = 8


def golden_loop_lcm(dtype=torch.float32, save=True, given_noise=None):
    """golden_loop's body (tiny nets) under LCMScheduler with classifier-free guidance (7.5) and without (1.0: as pipe:1031 the
    reference then runs the networks at batch B on the positive prompt only - the second half of g(32) - and uses the UNet output as it
    is), and the same guidance-free loop under DDIM and UniPC.  A CPU generator gives the LCM noise (tapped).  Stores the final latents,
    the latents entering every step and the (guided) eps.  `dtype=torch.float64, save=False` returns the same loops in float64; `given_noise` (an earlier result of this
    function) then hands every step the noise THAT run drew - a float64 generator draw is another sample, not another rounding."""
    from diffusers import LCMScheduler
    plain_unet, blob = build_tiny()
    cond_unet, _ = build_tiny(LCM_WCOND_DIM)
    plain_unet, cond_unet, blob = plain_unet.to(dtype), cond_unet.to(dtype), blob.to(dtype)
    c = TINY
    h = w = 8
    out = {}
    pipe = StableDiffusionBlobNetPipeline.__new__(StableDiffusionBlobNetPipeline)
    for tag, (cls, set_kw, guidance, (gs, ge), seed) in LCM_LOOPS.items():
        wcond = "wcond" in tag
        unet = cond_unet if wcond else plain_unet
        B = 2 if tag == "lcm_wcond_custom_3" else 1
        sch = {"lcm": lambda: LCMScheduler.from_config(SD15_SCHEDULER_JSON), "unipc": lambda: UniPCMultistepScheduler(**SD_SCHED),
               "ddim": lambda: DDIMScheduler(**SD_SCHED, clip_sample=False, set_alpha_to_one=False)}[cls]()
        sch.set_timesteps(**set_kw)
        steps = len(sch.timesteps)
        cfg = guidance > 1.0 and not wcond                                   # pipe:497
        R = 2 * B if cfg else B                                              # rows the networks see
        tcond = None
        if wcond:                                                            # pipe:987-993
            tcond = StableDiffusionBlobNetPipeline.get_guidance_scale_embedding(
                pipe, torch.tensor(guidance - 1).repeat(B), embedding_dim=LCM_WCOND_DIM).to(dtype)
            out[f"{tag}_timestep_cond"] = tcond.numpy()
        gen = torch.Generator().manual_seed(seed) if seed is not None else None
        latents = (g(31, B, 4, h, w) * sch.init_noise_sigma).to(dtype)
        prompt = g(32, 2 * B, 7, c["ctx"]).to(dtype)
        if not cfg:
            prompt = prompt[B:]
        fg_lat = (g(33, 1, 4, h, w) * 0.18215 * 5).repeat(R, 1, 1, 1).to(dtype)
        bg_lat = (g(34, 1, 4, h, w) * 0.18215 * 5).repeat(R, 1, 1, 1).to(dtype)
        ell = [[40.0, 42.0], [20.0, 30.0], 25.0]
        mean, cov = ref_inf.get_gs_from_ellipse(ell)
        nm, nc = ref_inf.normalize_gs(mean, cov, 64, 64)
        gs_score = splat_features(**ref_inf.get_blob_dict_from_norm_gs(nm, nc), score_size=(h, w), return_d_score=True)
        bg_s, fg_s = gs_score.unbind(dim=1)
        bg_s = bg_s.unsqueeze(1).repeat(R, 1, 1, 1).to(dtype)
        fg_s = fg_s.unsqueeze(1).repeat(R, 1, 1, 1).to(dtype)
        dino = g(35, 1, 1, c["feat"]).to(dtype)
        feats = pipe.splat_features_from_scores(fg_s, dino.repeat(R, 1, 1), size=h, channels_last=False)
        keep = [1.0 - float(i / steps < gs or (i + 1) / steps > ge) for i in range(steps)]
        eps_trace, lat_trace = [], []
        give = given_noise is not None and f"{tag}_noise" in given_noise
        ctx = _GiveNoise(LCM_MODULE, [torch.from_numpy(v).to(dtype) for v in given_noise[f"{tag}_noise"]]) if give else _TapNoise(LCM_MODULE)
        with ctx as tap:
            for i, t in enumerate(sch.timesteps):
                lat_trace.append(latents.numpy().copy())
                lmi = sch.scale_model_input(torch.cat([latents] * 2) if cfg else latents, t)       # pipe:1031-1032
                bi = pipe.construct_blobnet_input(lmi, fg_s, fg_lat, feats, background=False)
                d, m, u = blob(bi, t, conditioning_scale=1.0 * keep[i], return_dict=False)
                ui = pipe.construct_blobnet_input(lmi, bg_s, bg_lat, background=True)
                npred = unet(ui, t, encoder_hidden_states=prompt, timestep_cond=tcond,
                             down_block_add_samples=[x[..., -x.shape[-2]:] for x in d],
                             mid_block_add_sample=m[..., -m.shape[-2]:], up_block_add_samples=[x[..., -x.shape[-2]:] for x in u],
                             return_dict=False)[0]
                b_, c_, h_, w_ = npred.shape
                npred = npred[..., :h_, w_ // 2:]
                if cfg:                                                                             # pipe:1095-1098
                    nu, nt = npred.chunk(2)
                    npred = nu + guidance * (nt - nu)
                eps_trace.append(npred.numpy())
                step_kw = dict(generator=gen) if cls == "lcm" else {}
                latents = sch.step(npred, t, latents, return_dict=False, **step_kw)[0].to(dtype)
        if give:
            assert not tap.noises
            tap.drawn = [torch.from_numpy(v) for v in given_noise[f"{tag}_noise"]]
        assert len(tap.drawn) == (steps - 1 if cls == "lcm" else 0)
        out[f"{tag}_final"] = latents.numpy()
        out[f"{tag}_eps"] = np.stack(eps_trace)
        out[f"{tag}_lat"] = np.stack(lat_trace)
        out[f"{tag}_timesteps"] = sch.timesteps.numpy()
        out[f"{tag}_window"] = np.array([gs, ge])
        out[f"{tag}_kw"] = np.array(json.dumps(dict(cls=cls, set_timesteps=set_kw, guidance_scale=guidance, batch=B,
                                                    time_cond_proj_dim=LCM_WCOND_DIM if wcond else None)))
        if cls == "lcm":
            out[f"{tag}_noise"] = torch.stack(tap.drawn).numpy()
            out[f"{tag}_seed"] = np.array(seed)
        print(f"loop_lcm {tag} ({dtype}): {steps} steps, batch {R}, final std {latents.std():.4f}")
    if save:
        np.savez_compressed(os.path.join(OUT, "loop_tiny_lcm.npz"), **out)
    return out


def golden_unet_timecond():
    """The tiny UNet with time_cond_proj_dim = 8 (time_embedding.cond_proj.weight [16, 8], no bias) on golden_nets' "wide" inputs: its
    forward with a `timestep_cond` (the guidance-scale embeddings of 7.5 and 3.0, one per image, so that a wrong row shows), and without
    one (embeddings.py:576-579: no add).  Plus `get_guidance_scale_embedding` (pipe:456-483) itself for dims 8, 7 and 256 and the scales
    1.0, 3.0 and 7.5."""
    unet, blob = build_tiny(LCM_WCOND_DIM)
    assert tuple(unet.state_dict()["time_embedding.cond_proj.weight"].shape) == (TINY["boc"][0], LCM_WCOND_DIM)
    assert "time_embedding.cond_proj.bias" not in unet.state_dict()
    c = TINY
    pipe = StableDiffusionBlobNetPipeline.__new__(StableDiffusionBlobNetPipeline)
    emb = lambda scales, dim: StableDiffusionBlobNetPipeline.get_guidance_scale_embedding(
        pipe, torch.tensor([s_ - 1 for s_ in scales], dtype=torch.float32), embedding_dim=dim)
    out = {"scales": np.array([1.0, 3.0, 7.5])}
    for dim in (8, 7, 256):
        out[f"embedding_{dim}"] = emb([1.0, 3.0, 7.5], dim).numpy()
        one = torch.cat([StableDiffusionBlobNetPipeline.get_guidance_scale_embedding(pipe, torch.tensor(s_ - 1).repeat(1), embedding_dim=dim)
                         for s_ in (1.0, 3.0, 7.5)])                       # as pipe:990 builds it: torch.tensor(guidance_scale - 1).repeat(B)
        assert torch.equal(one, torch.from_numpy(out[f"embedding_{dim}"])), dim
    B, (h, w) = 2, (8, 16)
    x_b = g(11, B, 4 + 1 + c["feat"], h, w)
    t = torch.tensor(981)
    down, mid, up = blob(x_b, t, conditioning_scale=0.8, return_dict=False)
    x_u, ehs = g(12, B, 5, h, w), g(13, B, 7, c["ctx"])
    sq = (lambda r: r[..., -r.shape[-2]:])
    tcond = emb([7.5, 3.0], LCM_WCOND_DIM)
    res = lambda: dict(down_block_add_samples=[sq(r).clone() for r in down], mid_block_add_sample=sq(mid).clone(),
                       up_block_add_samples=[sq(r).clone() for r in up])
    out.update(blob_in=x_b.numpy(), unet_in=x_u.numpy(), ehs=ehs.numpy(), timestep=np.array(981), timestep_cond=tcond.numpy(),
               eps=unet(x_u, t, encoder_hidden_states=ehs, timestep_cond=tcond, return_dict=False, **res())[0].numpy(),
               eps_plain=unet(x_u, t, encoder_hidden_states=ehs, timestep_cond=tcond, return_dict=False)[0].numpy(),
               eps_nocond=unet(x_u, t, encoder_hidden_states=ehs, return_dict=False, **res())[0].numpy())
    for i, r in enumerate(down):
        out[f"down_{i}"] = sq(r).numpy()
    out["mid"] = sq(mid).numpy()
    for i, r in enumerate(up):
        out[f"up_{i}"] = sq(r).numpy()
    np.savez_compressed(os.path.join(OUT, "unet_tiny_timecond.npz"), **out)
    print("unet_timecond: eps std %.4f, cond delta %.4f" % (out["eps"].std(), np.abs(out["eps"] - out["eps_nocond"]).max()))


def lcm_loop_spread():
    """The reference's own fp32-versus-fp64 spread of golden_loop_lcm's final latents (max-abs / scale), printed per case."""
    a = golden_loop_lcm(save=False)
    b = golden_loop_lcm(torch.float64, save=False, given_noise=a)
    for tag in LCM_LOOPS:
        x, y = a[f"{tag}_final"].astype(np.float64), b[f"{tag}_final"].astype(np.float64)
        print(f"{tag}: reference fp32 vs fp64 final latents max-abs/scale {np.abs(x - y).max() / np.abs(y).max():.3e}")


def golden_pipeline_call_lcm():
    """The reference's own `__call__` (pipe:743-1166) with `LCMScheduler.from_config(pipeline.scheduler.config)` on the plain tiny
    components, 4 steps and a CPU `generator` (start latents, then the noise of three steps), with classifier-free guidance (7.5) and
    without (1.0: prompt_embeds holds the positive prompts only, the networks run at batch B); and on the components of a distilled LCM
    model (UNet with time_cond_proj_dim = 8) at guidance 7.5, which goes in as timestep_cond (pipe:987-993) with CFG off (pipe:497).
    Case = `ddim_neg2` of pipeline_call.npz
    with its own seeds; the images and scores are those of pipeline_call.npz."""
    from PIL import Image
    from diffusers import LCMScheduler
    from tests.common import FakeTokenizer, pipeline_cases
    unet, blob, vae, te, proc, dino = _tiny_pipeline_components()
    cond_unet = _tiny_pipeline_components(LCM_WCOND_DIM)[0]
    base = np.load(os.path.join(OUT, "pipeline_call.npz"))
    kw = dict(pipeline_cases()["ddim_neg2"], seed=2027, rng_seed=29)
    for k in ("scheduler", "guidance_scale"):
        kw.pop(k, None)
    seed, rng_seed = kw.pop("seed"), kw.pop("rng_seed")
    kw["num_inference_steps"] = 4
    src = DDIMScheduler(**SD_SCHED, clip_sample=False, set_alpha_to_one=False)
    pipe = StableDiffusionBlobNetPipeline(vae=vae, unet=unet, tokenizer=FakeTokenizer(), text_encoder=te, blobnet=blob, scheduler=src,
                                          safety_checker=None, dinov2_processor=proc, dinov2=dino, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    out = {"seed": np.array(seed), "rng_seed": np.array(rng_seed), "num_inference_steps": np.array(kw["num_inference_steps"])}
    for tag, guidance in (("cfg", 7.5), ("nocfg", 1.0), ("wcond", 7.5)):
        if tag == "wcond":
            pipe = StableDiffusionBlobNetPipeline(vae=vae, unet=cond_unet, tokenizer=FakeTokenizer(), text_encoder=te, blobnet=blob,
                                                  scheduler=src, safety_checker=None, dinov2_processor=proc, dinov2=dino,
                                                  requires_safety_checker=False)
            pipe.set_progress_bar_config(disable=True)
            assert pipe.unet.config.time_cond_proj_dim == LCM_WCOND_DIM
        pipe.scheduler = LCMScheduler.from_config(src.config)
        torch.manual_seed(rng_seed)
        with _TapNoise(LCM_MODULE) as noise:
            r = pipe(fg_image=Image.fromarray(base["fg"]), bg_image=Image.fromarray(base["bg"]), gs_score=torch.from_numpy(base["gs_score"]),
                     height=64, width=64, generator=torch.Generator().manual_seed(seed), output_type="latent", guidance_scale=guidance, **kw)
        assert len(noise.drawn) == kw["num_inference_steps"] - 1 and pipe.do_classifier_free_guidance == (tag == "cfg")
        out[f"{tag}_latents"] = r.images.numpy()
        out[f"{tag}_noise"] = torch.stack(noise.drawn).numpy()
        out[f"{tag}_timesteps"] = pipe.scheduler.timesteps.numpy()
        out[f"{tag}_guidance_scale"] = np.array(guidance)
        print(f"pipeline __call__ lcm {tag} on {out[f'{tag}_timesteps']}: latents std {out[f'{tag}_latents'].std():.4f}, noise "
              f"{out[f'{tag}_noise'].shape}")
    np.savez_compressed(os.path.join(OUT, "pipeline_call_lcm.npz"), **out)


# ------------------------------------------------------------------------------------------------ FreeU
FREEU = (0.9, 0.2, 1.5, 1.6)                 # (s1, s2, b1, b2)
FREEU_FILTER_ONLY = (0.9, 0.2, 1.0, 1.0)     # b = 1: only the Fourier filter acts (a scale-only implementation equals eps_off here)
FREEU_BAR = 1e-2                             # the GPU tests' bar (max-abs / scale); the variants must lie >= 10 x that apart
FREEU_GEOMETRIES = {"wide16": (2, 16, 32), "wide12": (2, 12, 24), "square16": (1, 16, 16)}      # UNet canvas (B, H, W)
FREEU_RES_SCALE = 0.1


def _freeu_residual_shapes(H, W):
    """(channels, h, w) of the 12 down, the mid and the 15 up residuals of the tiny UNet on an H x W canvas (the right-hand square
    slices the pipeline passes, pipe:1085-1087)."""
    boc = TINY["boc"]
    sizes, h, w = [], H, W
    for i in range(len(boc)):
        sizes.append((h, w))
        if i < len(boc) - 1:
            h, w = (h + 1) // 2, (w + 1) // 2
    down = [(boc[0],) + sizes[0]]
    for i in range(len(boc)):
        down += [(boc[i],) + sizes[i]] * 2
        if i < len(boc) - 1:
            down.append((boc[i],) + sizes[i + 1])
    rev, up = list(reversed(boc)), []
    for i in range(len(boc)):
        up += [(rev[i],) + sizes[len(boc) - 1 - i]] * 3
        if i < len(boc) - 1:
            up.append((rev[i],) + sizes[len(boc) - 2 - i])
    sq = lambda s: (s[0], s[1], min(s[1], s[2]))
    return [sq(s) for s in down], sq((boc[-1],) + sizes[-1]), [sq(s) for s in up]


def freeu_residuals(seed, B, H, W):
    """The residual tensors of a FreeU case: seeded normal draws times FREEU_RES_SCALE (tests/test_freeu_gpu.py regenerates them from the
    stored seed - 28 tensors per geometry are not stored)."""
    down, mid, up = _freeu_residual_shapes(H, W)
    mk = lambda i, s: g(seed + i, B, *s) * FREEU_RES_SCALE
    return [mk(i, s) for i, s in enumerate(down)], mk(100, mid), [mk(200 + i, s) for i, s in enumerate(up)]


def golden_freeu():
    """The tiny UNet of build_tiny() with the reference's `enable_freeu` (unet_2d_condition.py:839-861 -> apply_freeu, torch_utils.py:
    93-148), laid out like unet_tiny_timecond.npz: a 16 x 32 canvas (FreeU sites 2 x 4 and 4 x 8), a 12 x 24 canvas (2 x 3 and 3 x 6: odd
    and non-power-of-two sizes, where the reference's filter runs in fp32) and a square 16 x 16 one (2 x 2 and 4 x 4), each with residuals
    added as BlobNet's are (seeded stand-ins, freeu_residuals) and with (s1, s2, b1, b2) = FREEU; plus `eps_off` (FreeU disabled) and
    `eps_filter_only` (FREEU_FILTER_ONLY).  Asserts that both variants lie at least 10 x the GPU bar away from eps_off."""
    unet, _ = build_tiny()
    c = TINY
    out = {"freeu": np.array(FREEU), "freeu_filter_only": np.array(FREEU_FILTER_ONLY), "timestep": np.array(981),
           "res_scale": np.array(FREEU_RES_SCALE)}
    t = torch.tensor(981)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    for n, (name, (B, H, W)) in enumerate(FREEU_GEOMETRIES.items()):
        seed = 1000 * (n + 1)
        x_u, ehs = g(seed + 500, B, 5, H, W), g(seed + 501, B, 7, c["ctx"])
        down, mid, up = freeu_residuals(seed, B, H, W)
        res = lambda: dict(down_block_add_samples=[r.clone() for r in down], mid_block_add_sample=mid.clone(),
                           up_block_add_samples=[r.clone() for r in up])
        run = lambda: unet(x_u, t, encoder_hidden_states=ehs, return_dict=False, **res())[0].numpy()
        unet.disable_freeu()
        eps_off = run()
        unet.enable_freeu(*FREEU)
        eps = run()
        unet.enable_freeu(*FREEU_FILTER_ONLY)
        eps_filter = run()
        unet.disable_freeu()
        assert np.array_equal(run(), eps_off)
        out.update({f"{name}_unet_in": x_u.numpy(), f"{name}_ehs": ehs.numpy(), f"{name}_res_seed": np.array(seed),
                    f"{name}_eps": eps, f"{name}_eps_off": eps_off, f"{name}_eps_filter_only": eps_filter})
        r1, r2 = rel(eps, eps_off), rel(eps_filter, eps_off)
        print(f"freeu {name} ({B} x {H} x {W}): eps vs eps_off {r1:.3f} = {r1 / FREEU_BAR:.0f} x the bar, filter only vs eps_off {r2:.3f} = "
              f"{r2 / FREEU_BAR:.0f} x the bar, eps std {eps.std():.4f}")
        assert r1 >= 10 * FREEU_BAR and r2 >= 10 * FREEU_BAR, (name, r1, r2)
    np.savez_compressed(os.path.join(OUT, "unet_tiny_freeu.npz"), **out)
    print("unet_tiny_freeu.npz: %.1f KB" % (os.path.getsize(os.path.join(OUT, "unet_tiny_freeu.npz")) / 1024))


def golden_pipeline_call_freeu():
    """The reference's own `__call__` (pipe:743-1166) after `pipe.enable_freeu(*FREEU)` (pipeline_utils.py:1905-1925): DDIM, 3 steps, the
    case `ddim_neg2` of pipeline_call.npz with its own seeds, images and scores those of pipeline_call.npz.  Stores the final latents
    with FreeU on, with other values (`latents_other`) and with FreeU disabled again (`latents_off`), and the loop-entry tensors."""
    from PIL import Image
    from tests.common import FakeTokenizer, pipeline_cases
    unet, blob, vae, te, proc, dino = _tiny_pipeline_components()
    base = np.load(os.path.join(OUT, "pipeline_call.npz"))
    kw = dict(pipeline_cases()["ddim_neg2"], seed=2031, rng_seed=37)
    kw.pop("scheduler")
    kw["num_inference_steps"] = 3
    sch = DDIMScheduler(**SD_SCHED, clip_sample=False, set_alpha_to_one=False)
    pipe = StableDiffusionBlobNetPipeline(vae=vae, unet=unet, tokenizer=FakeTokenizer(), text_encoder=te, blobnet=blob, scheduler=sch,
                                          safety_checker=None, dinov2_processor=proc, dinov2=dino, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    entry = {"lat": []}

    def tap(fn, key):
        def wrapped(*a, **k_):
            r_ = fn(*a, **k_)
            if key == "lat":
                entry["lat"].append(r_.detach().clone())
            else:
                entry[key] = r_
            return r_
        return wrapped
    pipe.encode_prompt = tap(pipe.encode_prompt, "prompt")
    pipe.encode_latents = tap(pipe.encode_latents, "lat")
    pipe.encode_image_dinov2 = tap(pipe.encode_image_dinov2, "dino")
    seed, rng_seed = kw.pop("seed"), kw.pop("rng_seed")
    other = (0.6, 0.4, 1.2, 1.4)
    out = {"seed": np.array(seed), "rng_seed": np.array(rng_seed), "num_inference_steps": np.array(kw["num_inference_steps"]),
           "freeu": np.array(FREEU), "freeu_other": np.array(other)}

    def call():
        torch.manual_seed(rng_seed)
        return pipe(fg_image=Image.fromarray(base["fg"]), bg_image=Image.fromarray(base["bg"]), gs_score=torch.from_numpy(base["gs_score"]),
                    height=64, width=64, generator=torch.Generator().manual_seed(seed), output_type="latent", **kw).images.numpy()
    pipe.enable_freeu(*FREEU)
    out["latents"] = call()
    pe, ne = entry["prompt"]
    out["entry_prompt_embeds"], out["entry_negative_prompt_embeds"] = pe.numpy(), ne.numpy()
    out["entry_fg_latents"] = entry["lat"][0][:1].numpy()
    out["entry_bg_latents"] = entry["lat"][1][:1].numpy()
    out["entry_dino"] = entry["dino"].numpy()
    pipe.enable_freeu(*other)
    out["latents_other"] = call()
    pipe.disable_freeu()
    out["latents_off"] = call()
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    print("pipeline __call__ freeu: latents std %.4f; vs off %.3f, other vs on %.3f (max-abs / scale)" %
          (out["latents"].std(), rel(out["latents"], out["latents_off"]), rel(out["latents_other"], out["latents"])))
    assert rel(out["latents"], out["latents_off"]) >= 10 * FREEU_BAR and rel(out["latents_other"], out["latents"]) >= 10 * FREEU_BAR
    np.savez_compressed(os.path.join(OUT, "pipeline_call_freeu.npz"), **out)
    print("pipeline_call_freeu.npz: %.1f KB" % (os.path.getsize(os.path.join(OUT, "pipeline_call_freeu.npz")) / 1024))


# ------------------------------------------------------------------------------------------------ 4. pipeline loop
class _FakeVaeCfg:
    scaling_factor = 0.18215
    block_out_channels = (1, 1, 1, 1)


def golden_loop():
    """Drive the reference pipeline's own __call__ loop code on the tiny nets by calling its methods directly:
    construct_blobnet_input + blobnet + unet + CFG + scheduler.step exactly as pipe:1025-1102 does."""
    unet, blob = build_tiny()
    c = TINY
    h = w = 8
    B = 1
    out = {}
    pipe = StableDiffusionBlobNetPipeline.__new__(StableDiffusionBlobNetPipeline)   # only stateless helpers are used
    for sname in ("unipc", "ddim"):
        for steps, (gs, ge) in ((5, (0.0, 1.0)), (6, (0.0, 0.67))):
            sch = (UniPCMultistepScheduler(**SD_SCHED) if sname == "unipc"
                   else DDIMScheduler(**SD_SCHED, clip_sample=False, set_alpha_to_one=False))
            sch.set_timesteps(steps)
            latents = g(31, B, 4, h, w) * sch.init_noise_sigma
            prompt = g(32, 2 * B, 7, c["ctx"])
            fg_lat = (g(33, 1, 4, h, w) * 0.18215 * 5).repeat(2 * B, 1, 1, 1)
            bg_lat = (g(34, 1, 4, h, w) * 0.18215 * 5).repeat(2 * B, 1, 1, 1)
            ell = [[40.0, 42.0], [20.0, 30.0], 25.0]
            mean, cov = ref_inf.get_gs_from_ellipse(ell)
            nm, nc = ref_inf.normalize_gs(mean, cov, 64, 64)
            gs_score = splat_features(**ref_inf.get_blob_dict_from_norm_gs(nm, nc), score_size=(h, w),
                                      return_d_score=True)
            bg_s, fg_s = gs_score.unbind(dim=1)
            bg_s = bg_s.unsqueeze(1).repeat(2 * B, 1, 1, 1).float()
            fg_s = fg_s.unsqueeze(1).repeat(2 * B, 1, 1, 1).float()
            dino = g(35, 1, 1, c["feat"])
            feats = pipe.splat_features_from_scores(fg_s, dino.repeat(2 * B, 1, 1), size=h, channels_last=False)
            keep = [1.0 - float(i / steps < gs or (i + 1) / steps > ge) for i in range(steps)]
            eps_trace = []
            for i, t in enumerate(sch.timesteps):
                lmi = sch.scale_model_input(torch.cat([latents] * 2), t)
                cond = 1.0 * keep[i]
                bi = pipe.construct_blobnet_input(lmi, fg_s, fg_lat, feats, background=False)
                d, m, u = blob(bi, t, conditioning_scale=cond, return_dict=False)
                ui = pipe.construct_blobnet_input(lmi, bg_s, bg_lat, background=True)
                npred = unet(ui, t, encoder_hidden_states=prompt,
                             down_block_add_samples=[x[..., -x.shape[-2]:] for x in d],
                             mid_block_add_sample=m[..., -m.shape[-2]:],
                             up_block_add_samples=[x[..., -x.shape[-2]:] for x in u], return_dict=False)[0]
                b_, c_, h_, w_ = npred.shape
                npred = npred[..., :h_, w_ // 2:]
                nu, nt = npred.chunk(2)
                npred = nu + 7.5 * (nt - nu)
                eps_trace.append(npred.numpy())
                latents = sch.step(npred, t, latents, return_dict=False)[0]
            tag = f"{sname}_{steps}"
            out[f"{tag}_final"] = latents.numpy()
            out[f"{tag}_eps"] = np.stack(eps_trace)
            out[f"{tag}_window"] = np.array([gs, ge])
            if sname == "unipc" and steps == 5:
                out["gs_score"] = gs_score.numpy()
                out["ellipse"] = np.array([40.0, 42.0, 20.0, 30.0, 25.0])
            print(f"loop {tag}: final std {latents.std():.4f}")
    np.savez_compressed(os.path.join(OUT, "loop_tiny.npz"), **out)


def golden_fullsize_loop(variants=None):
    """The north star's own parity statement: a FREE-RUNNING 50-step 512x512 edit on the full-size SD-1.5 UNet +
    BlobNet (reference classes, CPU fp32, the loop body of pipe:1025-1102 as golden_loop drives it), bench.py's synthetic weights and
    inputs, CFG 7.5, guidance window [0, 0.9] (45 BlobNet-active steps + 5 UNet-only).  Only the final latents and three intermediate
    checkpoints per run are stored (4 x 64 KB).  ~25-40 min per run on 8 cores.  Variants: "<scheduler>:<conv_out_scale>", default
    all four of {unipc, ddim} x {1.0 (the benchmark's weights), 0.3 (synth.contractive_variant)}; runs already in the file are kept.
    tools/amplification_probe.py measured how much the edit amplifies a perturbation of its start latents: 2.6 (DDIM) / 3.2 (UniPC)
    on the benchmark's weights, 1.3 / 1.5 at conv_out_scale 0.3."""
    import time
    import bench
    variants = variants or ["unipc:1.0", "ddim:1.0", "unipc:0.3", "ddim:0.3"]
    path = os.path.join(OUT, "loop_fullsize.npz")
    out = dict(np.load(path)) if os.path.exists(path) else {}
    h = w = 64
    steps, ge = 50, 0.9
    inp = bench.synth_inputs(h, w)
    usd0, bsd0 = bench.synth_weights()
    with torch.device("meta"):
        unet = UNet2DConditionModel(in_channels=5, out_channels=4, cross_attention_dim=768, attention_head_dim=8)
        blob = BlobNetModel(in_channels=4, conditioning_channels=1025, cross_attention_dim=None, attention_head_dim=8)
    pipe = StableDiffusionBlobNetPipeline.__new__(StableDiffusionBlobNetPipeline)
    ell = [[361.1067, 367.8526], [85.4812, 103.6543], 87.3739]
    mean, cov = ref_inf.get_gs_from_ellipse(ell)
    nm, nc = ref_inf.normalize_gs(mean, cov, 512, 512)
    gs_score = splat_features(**ref_inf.get_blob_dict_from_norm_gs(nm, nc), score_size=(h, w), return_d_score=True)
    bg_s, fg_s = gs_score.unbind(dim=1)
    bg_s, fg_s = bg_s.unsqueeze(1).repeat(2, 1, 1, 1).float(), fg_s.unsqueeze(1).repeat(2, 1, 1, 1).float()
    fg_lat, bg_lat = inp["fg"].repeat(2, 1, 1, 1), inp["bg"].repeat(2, 1, 1, 1)
    feats = pipe.splat_features_from_scores(fg_s, inp["dino"].repeat(2, 1, 1), size=h, channels_last=False)
    loaded = None
    for var in variants:
        sname, scale = var.split(":")
        scale = float(scale)
        tag = f"{sname}_s{scale:g}"
        if f"{tag}_final" in out:
            print("have", tag)
            continue
        if loaded != scale:
            usd, bsd = synth.contractive_variant(usd0, bsd0, conv_out_scale=scale) if scale != 1.0 else (usd0, bsd0)
            unet.load_state_dict(usd, strict=True, assign=True)
            blob.load_state_dict(bsd, strict=True, assign=True)
            unet.eval(); blob.eval()
            loaded = scale
        sch = (UniPCMultistepScheduler(**SD_SCHED) if sname == "unipc" else DDIMScheduler(**SD_SCHED, clip_sample=False, set_alpha_to_one=False))
        sch.set_timesteps(steps)
        latents = inp["latents"] * sch.init_noise_sigma
        keep = [1.0 - float(i / steps < 0.0 or (i + 1) / steps > ge) for i in range(steps)]
        t0 = time.time()
        for i, t in enumerate(sch.timesteps):
            lmi = sch.scale_model_input(torch.cat([latents] * 2), t)
            bi = pipe.construct_blobnet_input(lmi, fg_s, fg_lat, feats, background=False)
            d, m, u = blob(bi, t, conditioning_scale=1.0 * keep[i], return_dict=False)
            ui = pipe.construct_blobnet_input(lmi, bg_s, bg_lat, background=True)
            npred = unet(ui, t, encoder_hidden_states=inp["prompt"], down_block_add_samples=[x[..., -x.shape[-2]:] for x in d],
                         mid_block_add_sample=m[..., -m.shape[-2]:], up_block_add_samples=[x[..., -x.shape[-2]:] for x in u],
                         return_dict=False)[0]
            npred = npred[..., :, npred.shape[-1] // 2:]
            nu, nt = npred.chunk(2)
            npred = nu + 7.5 * (nt - nu)
            latents = sch.step(npred, t, latents, return_dict=False)[0]
            if i + 1 in (1, 10, 25, 40) and scale == 1.0:          # (checkpoints only for the benchmark's own weights: 64 KB each)
                out[f"{tag}_x{i + 1}"] = latents.numpy().copy()
            print(f"{tag} step {i + 1}/{steps} |x| max {latents.abs().max():.2f} ({time.time() - t0:.0f} s)", flush=True)
        out[f"{tag}_final"] = latents.numpy().copy()
        out["window_end"] = np.float32(ge)
        np.savez_compressed(path, **out)                      # after every run: a later interruption keeps the finished ones
        print("wrote", tag, "->", path)


def _ref_loop(unet, blob, pipe, sch, steps, ge, latents, prompt, fg, bg, gs_score, dino, strength, h, keep_at=()):
    """The loop body of pipe:1025-1102 on the reference classes (one request, CFG 7.5); returns the final latents and checkpoints."""
    import time
    bg_s, fg_s = gs_score.unbind(dim=1)
    bg_s, fg_s = bg_s.unsqueeze(1).repeat(2, 1, 1, 1).float(), fg_s.unsqueeze(1).repeat(2, 1, 1, 1).float()
    fg_lat, bg_lat = fg.repeat(2, 1, 1, 1), bg.repeat(2, 1, 1, 1)
    feats = pipe.splat_features_from_scores(fg_s, dino.repeat(2, 1, 1), size=h, channels_last=False)
    sch.set_timesteps(steps)
    latents = latents * sch.init_noise_sigma
    keep = [1.0 - float(i / steps < 0.0 or (i + 1) / steps > ge) for i in range(steps)]
    cps, t0 = {}, time.time()
    for i, t in enumerate(sch.timesteps):
        lmi = sch.scale_model_input(torch.cat([latents] * 2), t)
        bi = pipe.construct_blobnet_input(lmi, fg_s, fg_lat, feats, background=False)
        d, m, u = blob(bi, t, conditioning_scale=float(strength) * keep[i], return_dict=False)
        ui = pipe.construct_blobnet_input(lmi, bg_s, bg_lat, background=True)
        npred = unet(ui, t, encoder_hidden_states=prompt, down_block_add_samples=[x[..., -x.shape[-2]:] for x in d],
                     mid_block_add_sample=m[..., -m.shape[-2]:], up_block_add_samples=[x[..., -x.shape[-2]:] for x in u],
                     return_dict=False)[0]
        npred = npred[..., :, npred.shape[-1] // 2:]
        nu, nt = npred.chunk(2)
        latents = sch.step(nu + 7.5 * (nt - nu), t, latents, return_dict=False)[0]
        if i + 1 in keep_at:
            cps[i + 1] = latents.numpy().copy()
        print(f"   step {i + 1}/{steps} |x| max {latents.abs().max():.2f} ({time.time() - t0:.0f} s)", flush=True)
    return latents.numpy().copy(), cps


def golden_config_loops(which=None):
    """multi-step FREE-RUNNING reference runs at the other BASELINE configurations (only C2 had one).
    (i) `c5`: 768 x 768 (canvas 96 x 192), batch 1, 10 DDIM steps, window [0, 0.9] on bench.py's synthetic weights / inputs;
    (ii) `c3_r0` / `c3_r1`: requests 0 (move, strength 1.0) and 1 (`remove`: strength 0.0, gs_score = (1, 0), inf:175-188) of the
    mixed-operation batch of tests/test_fullsize_loop_gpu.py::test_c3_*, each alone (the reference runs one edit per call), 10 UniPC
    steps.  Stored: final latents + checkpoints after steps 1 and 5.  ~45 s per 768^2 step and ~15 s per 512^2 step on 8 cores."""
    import bench
    which = which or ["c5", "c3_r0", "c3_r1"]
    path = os.path.join(OUT, "loop_configs.npz")
    out = dict(np.load(path)) if os.path.exists(path) else {}
    with torch.device("meta"):
        unet = UNet2DConditionModel(in_channels=5, out_channels=4, cross_attention_dim=768, attention_head_dim=8)
        blob = BlobNetModel(in_channels=4, conditioning_channels=1025, cross_attention_dim=None, attention_head_dim=8)
    usd, bsd = bench.synth_weights()
    unet.load_state_dict(usd, strict=True, assign=True)
    blob.load_state_dict(bsd, strict=True, assign=True)
    unet.eval(); blob.eval()
    pipe = StableDiffusionBlobNetPipeline.__new__(StableDiffusionBlobNetPipeline)
    steps, ge = 10, 0.9

    def ref_score(ell, W, H, h, w):
        mean, cov = ref_inf.get_gs_from_ellipse(ell)
        nm, nc = ref_inf.normalize_gs(mean, cov, W, H)
        return splat_features(**ref_inf.get_blob_dict_from_norm_gs(nm, nc), score_size=(h, w), return_d_score=True)

    for tag in which:
        if f"{tag}_final" in out:
            print("have", tag)
            continue
        print("running", tag, flush=True)
        if tag == "c5":
            h = w = 96
            inp = bench.synth_inputs(h, w)
            s = (8 * w) / 512.0
            score = ref_score([[361.1067 * s, 367.8526 * s], [85.4812 * s, 103.6543 * s], 87.3739], 8 * w, 8 * h, h, w)
            sch = DDIMScheduler(**SD_SCHED, clip_sample=False, set_alpha_to_one=False)
            final, cps = _ref_loop(unet, blob, pipe, sch, steps, ge, inp["latents"], inp["prompt"], inp["fg"], inp["bg"], score,
                                   inp["dino"], 1.0, h, keep_at=(1, 5))
        else:
            b = int(tag[-1])
            B, h, w = 8, 64, 64
            ells = [[[200.0 + 30 * i, 180.0 + 25 * i], [60.0 + 6 * i, 90.0 - 4 * i], 20.0 * i] for i in range(B)]
            strengths = [1.0, 0.0, 1.0, 1.2, 0.0, 1.0, 0.6, 1.0]
            score = ref_score(ells[b], 512, 512, h, w)
            if strengths[b] == 0.0:
                score[:, 0], score[:, 1] = 1.0, 0.0
            fg, bg = g(201, B, 4, h, w) * 0.18215 * 5, g(202, B, 4, h, w) * 0.18215 * 5
            dino, lat = g(203, B, 1, 1024), g(204, B, 4, h, w)
            neg, pos = g(205, 1, 77, 768).repeat(B, 1, 1), g(206, B, 77, 768)
            sch = UniPCMultistepScheduler(**SD_SCHED)
            final, cps = _ref_loop(unet, blob, pipe, sch, steps, ge, lat[b:b + 1], torch.cat([neg[b:b + 1], pos[b:b + 1]]),
                                   fg[b:b + 1], bg[b:b + 1], score, dino[b:b + 1], strengths[b], h, keep_at=(1, 5))
        out[f"{tag}_final"] = final
        for k, v in cps.items():
            out[f"{tag}_x{k}"] = v
        out["steps"], out["window_end"] = np.int32(steps), np.float32(ge)
        np.savez_compressed(path, **out)
        print("wrote", tag, "->", path, flush=True)


def golden_cpu_step_seconds():
    """ONE denoise step of the REAL reference (vendored diffusers UNet + BlobNet classes at CFG batch 2, fp32,
    pipe:1043-1090) timed beside the oracle's `noise_pred_step` on the same cores, same weights and inputs, interleaved (one warm-up
    each, then alternating, best of 2): tests/golden/cpu_step_seconds.json.  bench.py's cpu_baseline (kind "port") quotes the ratio
    so that the port is shown to cost what the reference's own path costs (it was 3x slower while the oracle materialised the
    attention scores instead of calling F.scaled_dot_product_attention)."""
    import time
    import bench
    from oracle.nets import NetConfig
    from oracle.pipeline import noise_pred_step
    h = w = 64
    inp = bench.synth_inputs(h, w)
    usd, bsd = bench.synth_weights()
    with torch.device("meta"):
        unet = UNet2DConditionModel(in_channels=5, out_channels=4, cross_attention_dim=768, attention_head_dim=8)
        blob = BlobNetModel(in_channels=4, conditioning_channels=1025, cross_attention_dim=None, attention_head_dim=8)
    unet.load_state_dict(usd, strict=True, assign=True)
    blob.load_state_dict(bsd, strict=True, assign=True)
    unet.eval(); blob.eval()
    pipe = StableDiffusionBlobNetPipeline.__new__(StableDiffusionBlobNetPipeline)
    ell = [[361.1067, 367.8526], [85.4812, 103.6543], 87.3739]
    mean, cov = ref_inf.get_gs_from_ellipse(ell)
    nm, nc = ref_inf.normalize_gs(mean, cov, 512, 512)
    gs_score = splat_features(**ref_inf.get_blob_dict_from_norm_gs(nm, nc), score_size=(h, w), return_d_score=True)
    bg_s, fg_s = gs_score.unbind(dim=1)
    bg_s, fg_s = bg_s.unsqueeze(1).repeat(2, 1, 1, 1).float(), fg_s.unsqueeze(1).repeat(2, 1, 1, 1).float()
    fg_lat, bg_lat = inp["fg"].repeat(2, 1, 1, 1), inp["bg"].repeat(2, 1, 1, 1)
    feats = pipe.splat_features_from_scores(fg_s, inp["dino"].repeat(2, 1, 1), size=h, channels_last=False)
    ucfg, bcfg = NetConfig(in_channels=5, cross_attention_dim=768), NetConfig(in_channels=1029, cross_attention_dim=None)
    x = inp["latents"]

    def ref_step(t):
        lmi = torch.cat([x] * 2)
        bi = pipe.construct_blobnet_input(lmi, fg_s, fg_lat, feats, background=False)
        d, m, u = blob(bi, t, conditioning_scale=1.0, return_dict=False)
        ui = pipe.construct_blobnet_input(lmi, bg_s, bg_lat, background=True)
        npred = unet(ui, t, encoder_hidden_states=inp["prompt"], down_block_add_samples=[r[..., -r.shape[-2]:] for r in d],
                     mid_block_add_sample=m[..., -m.shape[-2]:], up_block_add_samples=[r[..., -r.shape[-2]:] for r in u],
                     return_dict=False)[0]
        npred = npred[..., :, npred.shape[-1] // 2:]
        nu, nt = npred.chunk(2)
        return nu + 7.5 * (nt - nu)

    def port_step(t):
        return noise_pred_step(usd, ucfg, bsd, bcfg, x, t, inp["prompt"], fg_lat, bg_lat, fg_s, bg_s, feats, 1.0, 7.5)

    times = {"reference": [], "port": []}
    outs = {}
    for rnd in range(3):                                   # round 0 = warm-up of both
        for name, fn in (("reference", ref_step), ("port", port_step)):
            t0 = time.perf_counter()
            outs[name] = fn(torch.tensor(981))
            dt = time.perf_counter() - t0
            if rnd:
                times[name].append(round(dt, 3))
            print(f"round {rnd} {name}: {dt:.2f} s", flush=True)
    rel = float((outs["port"] - outs["reference"]).abs().max() / outs["reference"].abs().max())
    doc = dict(threads=torch.get_num_threads(), cpus=len(os.sched_getaffinity(0)), resolution="512x512",
               what="one BlobNet-active denoise step, BlobNet AND UNet at CFG batch 2, fp32, after one warm-up step; best of 2",
               reference_s=min(times["reference"]), port_s=min(times["port"]), samples=times,
               port_vs_reference_ratio=round(min(times["port"]) / min(times["reference"]), 3),
               guided_eps_max_abs_rel_port_vs_reference=rel)
    with open(os.path.join(OUT, "cpu_step_seconds.json"), "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


# ------------------------------------------------------------------------------------------------ 5. dinov2
def golden_dinov2():
    from transformers import Dinov2Config, Dinov2Model
    cfg = Dinov2Config(hidden_size=64, num_hidden_layers=3, num_attention_heads=4, image_size=70, patch_size=14,
                       mlp_ratio=4)
    model = Dinov2Model(cfg).eval()
    shapes = synth.dinov2_param_shapes(64, 3, 4, 14, 25)
    assert set(shapes.keys()) == set(model.state_dict().keys()), "dinov2 schema mismatch"
    model.load_state_dict(synth.synth_state_dict(shapes, 99), strict=True)
    out = {}
    for tag, s in (("native", 70), ("interp", 56)):
        x = g(41, 2, 3, s, s)
        out[f"{tag}_in"] = x.numpy()
        out[f"{tag}_pooled"] = model(pixel_values=x).pooler_output.numpy()
    np.savez_compressed(os.path.join(OUT, "dinov2_tiny.npz"), **out)
    print("dinov2: pooled std %.4f" % out["native_pooled"].std())


def _hf_sam_model(cfg, sd):
    """transformers' SamModel for one of the tiny configurations of tests/sam_common.py, holding the synth weights `sd`."""
    from transformers import SamConfig, SamMaskDecoderConfig, SamModel, SamPromptEncoderConfig, SamVisionConfig
    from tests import sam_common as sc
    C = cfg["out_channels"]
    vc = SamVisionConfig(hidden_size=cfg["hidden"], output_channels=C, num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                         image_size=cfg["image"], patch_size=cfg["patch"], window_size=cfg["window"],
                         global_attn_indexes=list(cfg["global_attn_indexes"]), mlp_dim=cfg["mlp_dim"], num_pos_feats=C // 2)
    pc = SamPromptEncoderConfig(hidden_size=C, image_size=cfg["image"], patch_size=cfg["patch"], mask_input_channels=16)
    mc = SamMaskDecoderConfig(hidden_size=C, num_hidden_layers=cfg["decoder_layers"], num_attention_heads=sc.DECODER_HEADS,
                              mlp_dim=cfg["decoder_mlp_dim"], iou_head_hidden_dim=cfg["iou_head_hidden_dim"])
    model = SamModel(SamConfig(vision_config=vc, prompt_encoder_config=pc, mask_decoder_config=mc)).eval()
    assert set(sd.keys()) == set(model.state_dict().keys()), set(sd.keys()) ^ set(model.state_dict().keys())
    model.load_state_dict(sd, strict=True)
    return model


def golden_sam():
    """tests/golden/sam_tiny.npz: transformers' SamModel (CPU, fp32, synth weights) on the two tiny configurations of tests/sam_common.py -
    image embeddings, low-res logits and IoU scores for two click sets, the final masks at a non-square original size, the same with the
    qkv biases x 8 (the padded-window case), and SamPredictor's preprocessing from transformers' SAM image processor."""
    from transformers import SamImageProcessor
    from tests import sam_common as sc
    out = {}
    hf_model = _hf_sam_model

    def run(tag, cfg, sd, masks, pixel_seed=7):
        S = cfg["image"]
        model = hf_model(cfg, sd)
        # (pixels on a 1/32 grid, stored as int8: three fp32 frames would not fit the size limit of a committed file)
        q8 = torch.clamp(torch.round(32 * g(cfg["seed"] + pixel_seed, 1, 3, S, S)), -127, 127)
        x = q8 / 32
        if masks:
            x[..., sc.INPUT_SIZE[0]:, :] = 0
            x[..., :, sc.INPUT_SIZE[1]:] = 0
        with torch.no_grad():
            emb = model.get_image_embeddings(x)
        out[f"{tag}_pixels_q8"], out[f"{tag}_emb"] = (32 * x).round().to(torch.int8).numpy(), emb.numpy()
        peak = float(emb.abs().max())
        assert 0.1 < peak < 100, f"{tag}: |embedding| max {peak}"
        out[f"{tag}_emb_absmax"] = np.float32(peak)
        for name, (pts, labs) in sc.CLICKS.items():
            for multi in (False, True):
                with torch.no_grad():
                    r = model(image_embeddings=emb, input_points=torch.tensor([[pts]]), input_labels=torch.tensor([[labs]]),
                              multimask_output=multi)
                low, iou = r.pred_masks[0, 0], r.iou_scores[0, 0]
                key = f"{tag}_{name}_{'multi' if multi else 'single'}"
                out[key + "_low"], out[key + "_iou"] = low.numpy(), iou.numpy()
                if masks:
                    logits = sc.postprocess(low, S, sc.INPUT_SIZE, sc.ORIGINAL_SIZE)
                    m = 1e-2 * float(logits.abs().max())
                    share = float((logits.abs() < m).float().mean())
                    assert share <= 0.10, f"{key}: {share:.3f} of the mask pixels lie within {m:.3e} of the threshold: pick another seed"
                    out[key + "_mask"], out[key + "_margin"], out[key + "_near_share"] = (logits > 0).numpy(), np.float32(m), np.float32(share)
        return emb

    def run_seeded(tag, cfg, sd, masks):
        """`run` with the first pixel seed whose masks pass the builder's margin assertion ("pick another seed")."""
        for pixel_seed in range(7, 47):
            try:
                emb = run(tag, cfg, sd, masks, pixel_seed)
            except AssertionError as e:
                if "pick another seed" not in str(e):
                    raise
                continue
            out[f"{tag}_pixel_seed"] = np.int32(pixel_seed)
            return emb
        raise AssertionError(f"{tag}: no pixel seed in 7 .. 46 keeps the masks clear of their threshold")

    run_seeded("a", sc.TINY_A, sc.weights_of(sc.TINY_A), True)
    run_seeded("b", sc.TINY_B, sc.weights_of(sc.TINY_B), False)
    # the padded-window case: qkv biases x 8 make the zero-padded tokens' keys and values matter.  How far the reference moves when those
    # tokens are masked out instead of attended to (the restatement of tests/sam_common.py, which tests/test_sam_cpu.py holds to this file):
    sd8 = sc.weights_of(sc.TINY_A, 8.0)
    emb8 = run_seeded("a8", sc.TINY_A, sd8, True)
    a = sc.TINY_A
    x8 = torch.from_numpy(out["a8_pixels_q8"]).float() / 32
    with torch.no_grad():
        same = sc.vision_encoder(x8, sd8, a["heads"], a["window"], a["global_attn_indexes"])
        masked = sc.vision_encoder(x8, sd8, a["heads"], a["window"], a["global_attn_indexes"], mask_padded=True)
    assert sc.rel_err(same, emb8) < 1e-5
    moved = sc.rel_err(masked, emb8) / 1e-2                       # in bars of the GPU tests (rel_err < 1e-2)
    assert moved > 10, f"masking the padded tokens moves the embeddings by only {moved:.1f} bars"
    out["a8_masked_padding_moves_bars"] = np.float32(moved)
    # SamPredictor.set_image's host side, from transformers' own SAM image processor (long side 64 keeps the fixture small)
    rng = np.random.Generator(np.random.PCG64(133))
    yy, xx = np.mgrid[0:200, 0:150]
    img = np.stack([127 + 100 * np.sin(xx / 9.0 + c) * np.cos(yy / 13.0 - c) for c in range(3)], -1) + rng.normal(0, 12, (200, 150, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    proc = SamImageProcessor(size={"longest_edge": 64}, pad_size={"height": 64, "width": 64})
    full = proc(images=img, return_tensors="np")
    raw = proc(images=img, do_rescale=False, do_normalize=False, do_pad=False, return_tensors="np")["pixel_values"][0]
    assert tuple(full["reshaped_input_sizes"][0]) == (64, 48) and raw.shape == (3, 64, 48)
    assert np.array_equal(raw, np.round(raw)) and raw.min() >= 0 and raw.max() <= 255
    out["predictor_pre_image"] = img
    out["predictor_pre_resized"] = raw.transpose(1, 2, 0).astype(np.uint8)
    out["predictor_pre_tensor"] = full["pixel_values"].astype(np.float32)
    path = os.path.join(OUT, "sam_tiny.npz")
    np.savez_compressed(path, **out)
    print("sam: %d arrays, %d bytes; |emb| max a %.3f b %.3f a8 %.3f; masked padding moves a8 by %.1f bars" % (
        len(out), os.path.getsize(path), out["a_emb_absmax"], out["b_emb_absmax"], out["a8_emb_absmax"], moved))
    assert os.path.getsize(path) < 1 << 20


AMG_OFFSET = 0.05          # synthetic weights give logits of magnitude ~1: the package's offset of 1.0 makes every stability score 0
AMG_STORED = (0, 5, 10, 15)


def _middle_gap(values):
    """The midpoint of the widest gap between neighbours in the middle half of the sorted values."""
    v = np.sort(np.asarray(values, dtype=np.float64))
    mid = v[len(v) // 4: len(v) - len(v) // 4]
    k = int(np.argmax(np.diff(mid)))
    return float((mid[k] + mid[k + 1]) / 2), float(mid[k + 1] - mid[k])


def golden_sam_amg():
    """tests/golden/sam_amg.npz: transformers' SamModel on fixture (a)'s stored pixels with ONE batched call of 16 single-point prompts (the
    4 x 4 grid over ORIGINAL_SIZE in the input frame), the quantities SamAutomaticMaskGenerator filters on from transformers' own helpers
    (image_processing_pil_sam) over the reference's logits at ORIGINAL_SIZE, and thresholds for the end-to-end test that sit in the widest
    gaps of the reference's values."""
    from transformers.models.sam.image_processing_pil_sam import _batched_mask_to_box, _build_point_grid, _compute_stability_score
    from blobctrl_amd import sam
    from tests import sam_common as sc
    cfg = sc.TINY_A
    z = np.load(os.path.join(OUT, "sam_tiny.npz"))
    model = _hf_sam_model(cfg, sc.weights_of(cfg))
    x = torch.from_numpy(z["a_pixels_q8"]).float() / 32
    H, W = sc.ORIGINAL_SIZE
    grid = _build_point_grid(4) * np.array([[W, H]], dtype=np.float64)                  # x fastest, (x, y) in the original image
    pts = sam.scale_points(grid, sc.ORIGINAL_SIZE, cfg["image"])                         # fp32 [16][2] in the input frame
    assert sam.preprocess_shape(H, W, cfg["image"]) == sc.INPUT_SIZE
    with torch.no_grad():
        emb = model.get_image_embeddings(x)
        assert sc.rel_err(emb, z["a_emb"]) < 1e-6
        r = model(image_embeddings=emb, input_points=torch.from_numpy(pts).reshape(1, 16, 1, 2), input_labels=torch.ones(1, 16, 1, dtype=torch.long),
                  multimask_output=True)
    low, iou = r.pred_masks[0], r.iou_scores[0]                                          # [16][3][64][64], [16][3]
    assert tuple(low.shape) == (16, 3, 64, 64) and tuple(iou.shape) == (16, 3)
    logits = sc.postprocess(low.flatten(0, 1), cfg["image"], sc.INPUT_SIZE, sc.ORIGINAL_SIZE)        # [48][H][W]
    stability = _compute_stability_score(logits, 0.0, AMG_OFFSET).numpy().astype(np.float32)
    binary = logits > 0.0
    boxes = _batched_mask_to_box(binary).numpy().astype(np.int32)
    areas = binary.flatten(1).sum(1).numpy().astype(np.int32)
    iou_flat = iou.flatten().numpy()
    # the chain on the reference's own numbers, with thresholds in the widest gaps: every stage must drop something and leave something
    iou_thr, iou_gap = _middle_gap(iou_flat)
    keep1 = np.nonzero(iou_flat > iou_thr)[0]
    stab_thr, stab_gap = _middle_gap(stability[keep1])
    keep2 = keep1[stability[keep1] >= stab_thr]
    b = boxes[keep2].astype(np.float64)
    pair = []
    for i in range(len(b)):
        for j in range(i + 1, len(b)):
            iw = max(0.0, min(b[i, 2], b[j, 2]) - max(b[i, 0], b[j, 0]))
            ih = max(0.0, min(b[i, 3], b[j, 3]) - max(b[i, 1], b[j, 1]))
            union = (b[i, 2] - b[i, 0]) * (b[i, 3] - b[i, 1]) + (b[j, 2] - b[j, 0]) * (b[j, 3] - b[j, 1]) - iw * ih
            pair.append(iw * ih / union)
    nms_thr = float(np.median(pair))
    keep3 = keep2[sam.box_nms(boxes[keep2], iou_flat[keep2], nms_thr)]
    msg = f"48 -> {len(keep1)} (IoU > {iou_thr:.4f}) -> {len(keep2)} (stability >= {stab_thr:.4f}) -> {len(keep3)} (NMS at {nms_thr:.4f})"
    # Both filters must drop something and leave something, and two masks at least must come out of the NMS.  The NMS itself cannot be made to
    # drop one here: on seeded weights nearly every mask touches all four borders, every pair of surviving boxes has IoU exactly 1, the median is
    # 1 and nothing is > 1 (the count is stored as `nms_dropped`; the geometry of box_nms is the unit test's, tests/test_sam_amg_cpu.py).
    assert 48 > len(keep1) > len(keep2) >= len(keep3) >= 2, msg + ": pick another seed"
    out = dict(grid=grid, points=pts, iou=iou.numpy(), low=low[list(AMG_STORED)].numpy(), stored=np.array(AMG_STORED, dtype=np.int32),
               stability=stability, boxes=boxes, areas=areas, offset=np.float32(AMG_OFFSET), pred_iou_thresh=np.float32(iou_thr),
               stability_score_thresh=np.float32(stab_thr), box_nms_thresh=np.float32(nms_thr), ref_kept=keep3.astype(np.int32),
               nms_dropped=np.int32(len(keep2) - len(keep3)))
    path = os.path.join(OUT, "sam_amg.npz")
    np.savez_compressed(path, **out)
    print("sam_amg: %s; gaps IoU %.4f stability %.4f; IoU %.3f .. %.3f, stability %.3f .. %.3f; %d bytes" % (
        msg, iou_gap, stab_gap, iou_flat.min(), iou_flat.max(), stability.min(), stability.max(), os.path.getsize(path)))
    assert os.path.getsize(path) < 400 << 10


def golden_blob_edit():
    """Pure-geometry functions of scripts/blobctrl_app.py (the app itself needs gradio / cv2 / SAM and loads models at import, so
    only the wanted function definitions are taken out of its source with `ast` and executed here; cv2.boundingRect is the one
    OpenCV call among them and is replaced by its definition - min / max of the non-zero pixels)."""
    import ast
    from PIL import Image
    src = open("/root/reference/scripts/blobctrl_app.py").read()
    want = ["normalize_ellipse", "composite_mask_and_image", "is_point_in_ellipse", "calculate_ellipse_vertices", "move_ellipse",
            "resize_blob_func", "rotate_blob_func", "get_object_region_from_mask"]
    tree = ast.parse(src)
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert len(body) == len(want)

    class _Gr:
        warnings = []

        @staticmethod
        def Warning(msg):
            _Gr.warnings.append(msg)

    class _Cv2:
        @staticmethod
        def boundingRect(m):
            ys, xs = np.nonzero(m)
            return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)
    ns = {"np": np, "Image": Image, "gr": _Gr, "cv2": _Cv2}
    exec(compile(ast.Module(body=body, type_ignores=[]), "blobctrl_app_subset", "exec"), ns)
    rng = np.random.Generator(np.random.PCG64(17))
    out = {"ellipses": [], "normalize": [], "vertices": [], "inside": [], "move": [], "resize": [], "rotate": []}
    ells = [((256.0, 256.0), (120.0, 80.0), 30.0), ((361.1067, 367.8526), (85.4812, 103.6543), 87.3739),
            ((40.0, 470.0), (300.0, 40.0), 135.0), ((256.0, 256.0), (1e-5, 1e-5), 0.0), ((100.0, 90.0), (60.0, 60.0), 179.0)]
    for e in ells:
        out["ellipses"].append([list(e[0]), list(e[1]), e[2]])
        out["normalize"].append([float(v) for v in ns["normalize_ellipse"](e, 512, 384)])
        out["vertices"].append(ns["calculate_ellipse_vertices"](e).tolist())
        pts = rng.uniform(0, 512, size=(12, 2))
        out["inside"].append([[float(p[0]), float(p[1]), bool(ns["is_point_in_ellipse"](p, e))] for p in pts])
        tp = rng.uniform(0, 512, size=(3, 2)).tolist()
        m = ns["move_ellipse"](e, tp)
        out["move"].append({"points": tp, "out": [list(m[0]), list(m[1]), m[2]]})
        for rt in (0, 1, 2):
            for f in (1.0, 0.5, 1.7, 6.0, 0.05):
                _Gr.warnings = []
                r, rf = ns["resize_blob_func"](e, f, 512, 512, rt)
                out["resize"].append({"ellipse": len(out["ellipses"]) - 1, "factor": f, "type": rt,
                                      "out": [list(r[0]), list(r[1]), r[2]], "factor_out": float(rf),
                                      "too_big": any("too big" in w for w in _Gr.warnings),
                                      "too_small": any("too small" in w for w in _Gr.warnings)})
        for deg in (0.0, 45.0, 170.0, -30.0):
            r, _ = ns["rotate_blob_func"](e, deg)
            out["rotate"].append({"ellipse": len(out["ellipses"]) - 1, "deg": deg, "out": [list(r[0]), list(r[1]), r[2]]})
    img = rng.integers(0, 256, size=(24, 32, 3)).astype(np.uint8)
    mask = np.zeros((24, 32), np.uint8)
    mask[5:14, 9:21] = 255
    mask[10:18, 15:25] = 128
    mask3 = np.stack([mask, mask, np.zeros_like(mask)], -1)
    comp = np.array(ns["composite_mask_and_image"](mask, img, masked_color=[255, 255, 255]))
    comp3 = np.array(ns["composite_mask_and_image"](mask3, img, masked_color=[0, 0, 0]))
    obj = np.array(ns["get_object_region_from_mask"](mask, img))
    out["image"] = img.tolist()
    out["mask"] = mask.tolist()
    out["composite_white"] = comp.tolist()
    out["composite_rgbmask_black"] = comp3.tolist()
    out["object_region"] = obj.tolist()
    with open(os.path.join(OUT, "blob_edit.json"), "w") as f:
        json.dump(out, f)
    print("blob edit:", len(out["resize"]), "resize cases,", sum(r["too_big"] for r in out["resize"]), "too big,",
          sum(r["too_small"] for r in out["resize"]), "too small")


def golden_clip_text():
    """CLIP text tower (transformers, third-party; call site pipe:599-611 incl. the clip_skip branch)."""
    from transformers import CLIPTextConfig, CLIPTextModel
    cfg = CLIPTextConfig(vocab_size=99, hidden_size=64, intermediate_size=128, num_hidden_layers=3, num_attention_heads=4,
                         max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5)
    model = CLIPTextModel(cfg).eval()
    shapes = synth.clip_text_param_shapes(99, 64, 3, 128, 77)
    # the on-disk SD-1.5 checkpoint (transformers 4.49 layout) prefixes every key with "text_model."; the transformers installed
    # here (5.x) dropped the prefix - same tensors
    have = {k for k in model.state_dict().keys() if "position_ids" not in k}
    pre = "" if any(k.startswith("text_model.") for k in have) else "text_model."
    assert set(shapes.keys()) == {pre + k for k in have}, "clip schema mismatch"
    sd = synth.synth_state_dict(shapes, 77)
    model.load_state_dict({k[len(pre):]: v for k, v in sd.items()}, strict=False)
    rng = np.random.Generator(np.random.PCG64(5))
    ids = torch.from_numpy(rng.integers(1, 98, size=(2, 77)).astype(np.int64))
    ids[:, 0] = 0
    ids[0, 20:] = 98                                       # eos padding pattern
    out = {"ids": ids.numpy()}
    with torch.no_grad():
        r = model(ids, output_hidden_states=True)
    out["last_hidden_state"] = r[0].numpy()
    fln = model.text_model.final_layer_norm if hasattr(model, "text_model") else model.final_layer_norm
    out["clip_skip_1"] = fln(r.hidden_states[-2]).detach().numpy()                                    # pipe:604-611
    short = ids[:, :16].clone()
    with torch.no_grad():
        out["short_ids"] = short.numpy()
        out["short_last_hidden_state"] = model(short)[0].numpy()
    np.savez_compressed(os.path.join(OUT, "clip_text_tiny.npz"), **out)
    print("clip text: last_hidden std %.4f" % out["last_hidden_state"].std())


# ------------------------------------------------------------------------------------------------ 6. VAE
def golden_vae():
    from diffusers import AutoencoderKL
    with torch.device("meta"):
        full = AutoencoderKL(in_channels=3, out_channels=3, down_block_types=("DownEncoderBlock2D",) * 4,
                             up_block_types=("UpDecoderBlock2D",) * 4, block_out_channels=(128, 256, 512, 512),
                             layers_per_block=2, latent_channels=4, norm_num_groups=32, sample_size=512)
    sh = synth.vae_param_shapes()
    ref = {k: tuple(v.shape) for k, v in full.state_dict().items()}
    assert set(ref) == set(sh) and all(ref[k] == tuple(sh[k]) for k in ref), "VAE schema mismatch"
    print(f"full-size VAE: {len(ref)} tensors, {sum(int(np.prod(v)) for v in ref.values())/1e6:.1f} M params - schema OK")
    boc = (32, 32, 64, 64)
    vae = AutoencoderKL(in_channels=3, out_channels=3, down_block_types=("DownEncoderBlock2D",) * 4,
                        up_block_types=("UpDecoderBlock2D",) * 4, block_out_channels=boc, layers_per_block=2,
                        latent_channels=4, norm_num_groups=8, sample_size=32).eval()
    tsh = synth.vae_param_shapes(boc, 2, 4)
    assert set(tsh) == set(vae.state_dict().keys())
    vae.load_state_dict(synth.synth_state_dict(tsh, 21), strict=True)
    out = {}
    x = g(51, 2, 3, 32, 48).clamp(-1, 1)
    post = vae.encode(x).latent_dist
    out["img"] = x.numpy()
    out["moments"] = post.parameters.numpy()
    z = g(52, 2, 4, 4, 6)
    out["z"] = z.numpy()
    out["decoded"] = vae.decode(z, return_dict=False)[0].numpy()
    gen = torch.Generator().manual_seed(5)
    noise = torch.randn(post.mean.shape, generator=gen)
    gen = torch.Generator().manual_seed(5)
    out["noise"] = noise.numpy()
    out["sample"] = post.sample(generator=gen).numpy()
    np.savez_compressed(os.path.join(OUT, "vae_tiny.npz"), **out)
    print("vae: decoded std %.4f moments std %.4f" % (out["decoded"].std(), out["moments"].std()))


# cases of vae_tiled.npz: tag -> (latent h, w, batch, tile_overlap_factor); tile sizes 64 / 8 throughout
VAE_TILED_CASES = {"A": (16, 12, 2, 0.25), "B": (10, 8, 1, 0.5), "C": (4, 12, 1, 0.25), "Cp": (12, 4, 1, 0.25), "D": (8, 8, 1, 0.25)}


def golden_vae_tiled():
    """The reference AutoencoderKL with enable_tiling() (tiled_decode / tiled_encode, autoencoder_kl.py:340-442) on golden_vae's tiny VAE,
    tile_sample_min_size 64 and tile_latent_min_size 8: tiled `decoded` of a latent and tiled `moments` of an image of the matching size
    per case.  The tiles the reference cut are RECORDED, not recomputed: forward hooks on its decoder / encoder log every tile's input
    and output shape in call order (row-major), and the origin of a tile in the result is the running sum of the cropped pieces the
    reference concatenated.  Case D is below the tile size: tiling is enabled and not triggered (bit-equal to the plain result)."""
    from diffusers import AutoencoderKL
    boc = (32, 32, 64, 64)
    vae = AutoencoderKL(in_channels=3, out_channels=3, down_block_types=("DownEncoderBlock2D",) * 4,
                        up_block_types=("UpDecoderBlock2D",) * 4, block_out_channels=boc, layers_per_block=2,
                        latent_channels=4, norm_num_groups=8, sample_size=32).eval()
    vae.load_state_dict(synth.synth_state_dict(synth.vae_param_shapes(boc, 2, 4), 21), strict=True)
    assert (vae.tile_sample_min_size, vae.tile_latent_min_size, vae.tile_overlap_factor, vae.use_tiling, vae.use_slicing) == (32, 4, 0.25, False, False)
    vae.tile_sample_min_size, vae.tile_latent_min_size = 64, 8
    log = []
    hooks = [m.register_forward_hook(lambda mod, args, res: log.append((tuple(args[0].shape[2:]), tuple(res.shape[2:]))))
             for m in (vae.decoder, vae.encoder)]

    def record(limit, result_hw, grid_w):
        """[y0-free] tiles in call order -> per tile [in_h, in_w, out_h, out_w, oy, ox]; the grid is `grid_w` tiles wide"""
        rows, oy = [], 0
        for k, (i_hw, o_hw) in enumerate(log):
            if k % grid_w == 0:
                ox = 0
            rows.append([i_hw[0], i_hw[1], o_hw[0], o_hw[1], oy, ox])
            ox += min(o_hw[1], limit)
            if k % grid_w == grid_w - 1:
                oy += min(o_hw[0], limit)
        assert (oy, ox) == tuple(result_hw), (oy, ox, result_hw)
        return np.array(rows, np.int32)

    out, meta = {}, {}
    for k, (tag, (h, w, B, f)) in enumerate(VAE_TILED_CASES.items()):
        vae.tile_overlap_factor = f
        z = g(520 + 6 * k, B, 4, h, w)
        x = g(540 + 6 * k, B, 3, 8 * h, 8 * w).clamp(-1, 1)
        vae.disable_tiling()
        plain_dec, plain_mom = vae.decode(z, return_dict=False)[0], vae.encode(x).latent_dist.parameters
        vae.enable_tiling()
        del log[:]
        dec = vae.decode(z, return_dict=False)[0]
        n_dec = len(log)
        mom = vae.encode(x).latent_dist.parameters
        out[f"{tag}_z"], out[f"{tag}_img"], out[f"{tag}_decoded"], out[f"{tag}_moments"] = z.numpy(), x.numpy(), dec.numpy(), mom.numpy()
        m = dict(latent=[h, w], batch=B, f=f, tile_sample_min_size=64, tile_latent_min_size=8, decoded_shape=list(dec.shape),
                 moments_shape=list(mom.shape))
        if tag == "D":
            assert n_dec == 1 and len(log) == 2 and torch.equal(dec, plain_dec) and torch.equal(mom, plain_mom)
            m["tiled"] = False
        else:
            grid_w = len(range(0, w, int(8 * (1 - f))))
            assert len(log) == 2 * n_dec and n_dec % grid_w == 0 and n_dec > 1
            enc_log, log[:] = log[n_dec:], log[:n_dec]
            out[f"{tag}_decode_tiles"] = record(64 - int(64 * f), dec.shape[2:], grid_w)
            log[:] = enc_log
            out[f"{tag}_encode_tiles"] = record(8 - int(8 * f), mom.shape[2:], grid_w)
            m["tiled"], m["grid"] = True, [n_dec // grid_w, grid_w]
            sc = dec.abs().max().item()
            m["tiled_vs_plain_max_abs_over_scale"] = (dec - plain_dec).abs().max().item() / sc
            print(f"vae_tiled {tag}: {n_dec} tiles, decode tiled-vs-plain {m['tiled_vs_plain_max_abs_over_scale']:.3f} of scale, "
                  f"moments {(mom - plain_mom).abs().max().item() / mom.abs().max().item():.3f}")
        meta[tag] = m
    for hk in hooks:
        hk.remove()
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(OUT, "vae_tiled.npz")
    np.savez_compressed(path, **out)
    print("vae_tiled: %d arrays, %.1f KB" % (len(out), os.path.getsize(path) / 1024))


def golden_lora_keys():
    """Key renaming + alpha defaults of the reference LoRA loader (peft itself is absent here, so only the parts that live in the
    vendored diffusers tree are pinned: convert_unet_state_dict_to_peft and get_peft_kwargs)."""
    from diffusers.utils.state_dict_utils import convert_unet_state_dict_to_peft
    from diffusers.utils.peft_utils import get_peft_kwargs
    mods = ["down_blocks.0.attentions.0.transformer_blocks.0.attn1", "mid_block.attentions.0.transformer_blocks.0.attn2",
            "up_blocks.3.attentions.2.transformer_blocks.0.attn1.processor"]
    keys = []
    for m in mods:
        for proj in ("to_q", "to_k", "to_v", "to_out"):
            for d in ("down", "up"):
                keys.append(f"{m}.{proj}_lora.{d}.weight")
    keys += ["conv_in.lora.down.weight", "conv_in.lora.up.weight", "down_blocks.1.resnets.0.conv1.lora.down.weight",
             "down_blocks.1.resnets.0.conv1.lora.up.weight", "down_blocks.0.attentions.0.proj_in.lora_A.weight",
             "down_blocks.0.attentions.0.proj_in.lora_B.weight", "up_blocks.1.attentions.0.transformer_blocks.0.ff.net.2.lora.down.weight",
             "up_blocks.1.attentions.0.transformer_blocks.0.ff.net.2.lora.up.weight",
             "mid_block.attentions.0.transformer_blocks.0.attn1.to_out.0.lora_A.weight"]
    conv = convert_unet_state_dict_to_peft({k: i for i, k in enumerate(keys)})
    out = {"pairs": [[k, nk] for k, nk in zip(keys, conv.keys())]}
    # alpha / rank defaults: ranks in file order 4, 8, 4, 4 without alphas; then with alphas
    peft_sd = {"a.lora_A.weight": 0, "a.lora_B.weight": 0, "b.lora_A.weight": 0, "b.lora_B.weight": 0,
               "c.lora_A.weight": 0, "c.lora_B.weight": 0}
    ranks = {"a.lora_B.weight": 8, "b.lora_B.weight": 4, "c.lora_B.weight": 4}
    out["kwargs_no_alpha"] = {k: v for k, v in get_peft_kwargs(ranks, None, peft_sd).items() if k != "target_modules"}
    alphas = {"a.lora_A.weight.alpha": 16.0, "b.lora_A.weight.alpha": 4.0, "c.lora_A.weight.alpha": 4.0}
    out["kwargs_alpha"] = {k: v for k, v in get_peft_kwargs(ranks, alphas, peft_sd).items() if k != "target_modules"}
    with open(os.path.join(OUT, "lora_keys.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("lora keys:", len(out["pairs"]), "pairs;", out["kwargs_no_alpha"], out["kwargs_alpha"])


def golden_lora_kohya():
    """kohya / sd-scripts key names of every LoRA-targetable module of the SD-1.5 UNet (Linear: to_q/k/v, to_out.0, proj_in/out,
    ff.net.0.proj, ff.net.2, time_emb_proj; Conv2d: conv1, conv2, conv_shortcut, down/upsamplers.0.conv) and of CLIP-L (12 x 6), through the
    reference's `_convert_non_diffusers_lora_to_diffusers` and its peft key conversion (convert_unet_state_dict_to_peft for the UNet,
    convert_state_dict_to_diffusers + convert_state_dict_to_peft for the text encoder: lora_pipeline.py:317-320).  Recorded per module:
    the kohya name, the final module name, the network_alphas key the conversion emits and the module whose down weight that key names.
    For the UNet, `get_peft_kwargs` also says which module the alpha lands on (`alpha_pattern`); its text-encoder branch
    (peft_utils.py:176) cuts attention keys back to `...self_attn`, which names no LoRA layer, so that column is recorded for the UNet only."""
    from diffusers.loaders.lora_conversion_utils import _convert_non_diffusers_lora_to_diffusers
    from diffusers.utils.peft_utils import get_peft_kwargs
    from diffusers.utils.state_dict_utils import (convert_state_dict_to_diffusers, convert_state_dict_to_peft,
                                                  convert_unet_state_dict_to_peft)
    us = synth.trunk_param_shapes(5, (320, 640, 1280, 1280), 2, 768, 4, blobnet=False)
    leaf = ("to_q", "to_k", "to_v", "to_out.0", "proj_in", "proj_out", "ff.net.0.proj", "ff.net.2", "time_emb_proj", "conv1", "conv2",
            "conv_shortcut", "downsamplers.0.conv", "upsamplers.0.conv")
    unet_mods = [k[: -len(".weight")] for k in us if k.endswith(".weight") and k[: -len(".weight")].endswith(leaf)]
    te_mods = [f"text_model.encoder.layers.{i}.{m}" for i in range(12)
               for m in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "mlp.fc1", "mlp.fc2")]
    names = [("unet", "lora_unet_" + m.replace(".", "_"), m) for m in unet_mods]
    names += [("text_encoder", "lora_te_" + m.replace(".", "_"), m) for m in te_mods]
    sd = {}
    for i, (_, k, _) in enumerate(names):                     # down = 3 i, up = 3 i + 1, alpha = 3 i + 2: every value names its key
        sd[k + ".lora_down.weight"], sd[k + ".lora_up.weight"], sd[k + ".alpha"] = 3 * i, 3 * i + 1, torch.tensor(float(3 * i + 2))
    conv, alphas = _convert_non_diffusers_lora_to_diffusers(dict(sd))
    final = {"unet": convert_unet_state_dict_to_peft({k[len("unet."):]: v for k, v in conv.items() if k.startswith("unet.")}),
             "text_encoder": convert_state_dict_to_peft(convert_state_dict_to_diffusers(
                 {k[len("text_encoder."):]: v for k, v in conv.items() if k.startswith("text_encoder.")}))}
    down_of = {v: k for k, v in conv.items()}                 # value -> key after the first conversion
    where = {m: {v: k for k, v in d.items()} for m, d in final.items()}
    alpha_key = {v: k for k, v in alphas.items()}
    # get_peft_kwargs(is_unet=True): two extra entries share a value, so that every real alpha differs from the most common one
    ua = convert_unet_state_dict_to_peft({k[len("unet."):]: v for k, v in alphas.items() if k.startswith("unet.")})
    ua.update({"pad0.alpha": -1.0, "pad1.alpha": -1.0})
    pattern = {v: k for k, v in get_peft_kwargs({"x.lora_B.weight": 4}, ua, {"x.lora_A.weight": 0})["alpha_pattern"].items()}
    entries = []
    for i, (model, k, want) in enumerate(names):
        dk, uk = where[model][3 * i], where[model][3 * i + 1]
        assert dk.endswith(".lora_A.weight") and uk == dk.replace(".lora_A.", ".lora_B."), (k, dk, uk)
        ak = alpha_key[float(3 * i + 2)]
        base = ak[: -len(".alpha")]
        owners = [j for j in range(len(names)) if down_of[3 * j] == base or down_of[3 * j].startswith(base + ".")]
        assert len(owners) == 1, (ak, owners)
        j = owners[0]
        e = {"kohya": k, "model": model, "module": dk[: -len(".lora_A.weight")], "alpha_key": ak,
             "alpha_module": where[names[j][0]][3 * j][: -len(".lora_A.weight")]}
        if model == "unet":
            e["peft_alpha_pattern"] = pattern[float(3 * i + 2)]
        assert e["module"] == want, (k, e["module"], want)    # (the kohya name is the path with "." -> "_": the conversion must undo it)
        entries.append(e)
    with open(os.path.join(OUT, "lora_kohya_keys.json"), "w") as f:
        json.dump({"entries": entries}, f, indent=0)
    print("lora kohya keys:", len(entries), "modules,", sum(e["model"] == "unet" for e in entries), "in the UNet")


def golden_lora_merge():
    """The adapter arithmetic as the REFERENCE tree states it (peft is absent, but the vendored diffusers keeps its
    own LoRA layers): D/models/lora.py LoRALinearLayer / LoRAConv2dLayer forward (runtime branch: base(x) + lora_scale * up(down(x))
    [* network_alpha / rank]) and LoRACompatibleLinear / LoRACompatibleConv._fuse_lora (w + lora_scale * (alpha / r) * up . down).
    Linear and Conv2d 3x3, with and without network_alpha.  Stored: the factors, the input, the reference's runtime output, its fused
    weight and the fused layer's output."""
    import warnings
    from diffusers.models.lora import LoRACompatibleConv, LoRACompatibleLinear, LoRAConv2dLayer, LoRALinearLayer
    out = {}
    warnings.simplefilter("ignore")
    for tag, alpha in (("noalpha", None), ("alpha", 2.0)):
        # Linear 24 -> 20, rank 4
        lin = LoRACompatibleLinear(24, 20, bias=True)
        lin.weight.data = g(901, 20, 24) * 0.2
        lin.bias.data = g(902, 20) * 0.1
        ll = LoRALinearLayer(24, 20, rank=4, network_alpha=alpha)
        ll.down.weight.data = g(903, 4, 24) * 0.3
        ll.up.weight.data = g(904, 20, 4) * 0.3
        lin.set_lora_layer(ll)
        x = g(905, 3, 7, 24)
        y_rt = lin(x, 0.7)
        w0 = lin.weight.data.clone()
        lin._fuse_lora(lora_scale=0.7)
        y_f = lin(x)
        out.update({f"lin_{tag}_w": w0.numpy(), f"lin_{tag}_b": lin.bias.data.numpy(), f"lin_{tag}_down": ll.down.weight.data.numpy(),
                    f"lin_{tag}_up": ll.up.weight.data.numpy(), f"lin_{tag}_x": x.numpy(), f"lin_{tag}_y_runtime": y_rt.numpy(),
                    f"lin_{tag}_w_fused": lin.weight.data.numpy(), f"lin_{tag}_y_fused": y_f.numpy()})
        # Conv2d 3x3 6 -> 8, rank 4 (down is 3x3, up is 1x1: lora.py:275-278)
        cv = LoRACompatibleConv(6, 8, kernel_size=3, padding=1, bias=True)
        cv.weight.data = g(911, 8, 6, 3, 3) * 0.2
        cv.bias.data = g(912, 8) * 0.1
        cl = LoRAConv2dLayer(6, 8, rank=4, kernel_size=(3, 3), stride=(1, 1), padding=1, network_alpha=alpha)
        cl.down.weight.data = g(913, 4, 6, 3, 3) * 0.3
        cl.up.weight.data = g(914, 8, 4, 1, 1) * 0.3
        cv.set_lora_layer(cl)
        xc = g(915, 2, 6, 5, 9)
        y_rt = cv(xc, 0.7)
        w0 = cv.weight.data.clone()
        cv._fuse_lora(lora_scale=0.7)
        y_f = cv(xc)
        out.update({f"conv_{tag}_w": w0.numpy(), f"conv_{tag}_b": cv.bias.data.numpy(), f"conv_{tag}_down": cl.down.weight.data.numpy(),
                    f"conv_{tag}_up": cl.up.weight.data.numpy(), f"conv_{tag}_x": xc.numpy(), f"conv_{tag}_y_runtime": y_rt.numpy(),
                    f"conv_{tag}_w_fused": cv.weight.data.numpy(), f"conv_{tag}_y_fused": y_f.numpy()})
        for k in ("lin", "conv"):
            d = np.abs(out[f"{k}_{tag}_y_runtime"] - out[f"{k}_{tag}_y_fused"]).max()
            assert d < 1e-5, (k, tag, d)
    out["lora_scale"] = np.float32(0.7)
    out["network_alpha"] = np.float32(2.0)
    np.savez_compressed(os.path.join(OUT, "lora_merge.npz"), **out)
    print("lora merge:", sorted(out)[:4], "...")


def golden_blob_edit_cv():
    """OpenCV outputs the REFERENCE ITSELF holds (cv2 is absent here): for every demo under assets/results/demo the SAM mask
    (ori_result_gallery_2.png), the filled ellipse mask (ori_result_gallery_3.png = cv2.ellipse(.., 255, -1), app:717) and the state's
    first ellipse (= cv2.fitEllipse(convexHull(contours)) enlarged by the initial factor 1.05, app:382-389,902).  Stored as packed
    bit masks + the ellipse parameters; `fit_pinned` lists the demos whose first ellipse is the unedited fit x 1.05."""
    from PIL import Image
    root = "/root/reference/assets/results/demo"
    out = {}
    names = sorted(d for d in os.listdir(root) if os.path.exists(os.path.join(root, d, "state", "state.json")))
    for name in names:
        st = json.load(open(os.path.join(root, name, "state", "state.json")))
        e = st["ellipse_lists"][0][0]
        out[f"{name}_ellipse0"] = np.array([e[0][0], e[0][1], e[1][0], e[1][1], e[2]], np.float64)
        for idx, key in ((2, "mask"), (3, "filled")):
            im = np.array(Image.open(os.path.join(root, name, "ori_result_gallery", f"ori_result_gallery_{idx}.png")).convert("RGB")).astype(np.int32)
            out[f"{name}_{key}"] = np.packbits(im.sum(-1) > 3 * 127)               # (the gallery files went through a lossy codec)
            out[f"{name}_shape"] = np.array(im.shape[:2])
    out["names"] = np.array(names)
    out["enlarge_factor"] = np.float64(1.05)
    np.savez_compressed(os.path.join(OUT, "blob_edit_cv.npz"), **out)
    print("blob_edit_cv:", names, os.path.getsize(os.path.join(OUT, "blob_edit_cv.npz")) // 1024, "KB")


def _tiny_pipeline_components(time_cond_proj_dim=None):
    """The reference classes of golden_pipeline_call on the tiny weights: (unet, blobnet, vae, text encoder, DINOv2 processor, DINOv2)."""
    from diffusers import AutoencoderKL
    from transformers import BitImageProcessor, CLIPTextConfig, CLIPTextModel, Dinov2Config, Dinov2Model
    from tests.common import PIPE, tiny_pipeline_weights
    c = TINY
    unet5, blob = build_tiny(time_cond_proj_dim)
    # the script's construction (inf:229-249): a 4-channel UNet whose conv_in is replaced by a 5-channel one; config.in_channels stays 4
    unet = UNet2DConditionModel(in_channels=4, out_channels=4, block_out_channels=c["boc"], norm_num_groups=c["groups"],
                                attention_head_dim=c["heads"], cross_attention_dim=c["ctx"], layers_per_block=2,
                                time_cond_proj_dim=time_cond_proj_dim)
    unet.conv_in = torch.nn.Conv2d(5, unet.conv_in.out_channels, kernel_size=3, stride=1, padding=1)
    unet.load_state_dict(unet5.state_dict(), strict=True)
    unet.eval()
    assert unet.config.in_channels == 4
    vsd, csd, dsd = tiny_pipeline_weights()
    vae = AutoencoderKL(in_channels=3, out_channels=3, down_block_types=("DownEncoderBlock2D",) * 4,
                        up_block_types=("UpDecoderBlock2D",) * 4, block_out_channels=PIPE["vae_boc"], layers_per_block=2,
                        latent_channels=4, norm_num_groups=PIPE["vae_groups"], sample_size=32).eval()
    vae.load_state_dict(vsd, strict=True)
    pc = PIPE["clip"]
    te = CLIPTextModel(CLIPTextConfig(vocab_size=pc["vocab"], hidden_size=pc["hidden"], intermediate_size=pc["inter"],
                                      num_hidden_layers=pc["layers"], num_attention_heads=pc["heads"], max_position_embeddings=77,
                                      hidden_act="quick_gelu", layer_norm_eps=1e-5)).eval()
    have = {k for k in te.state_dict().keys() if "position_ids" not in k}
    pre = "" if any(k.startswith("text_model.") for k in have) else "text_model."
    assert set(csd.keys()) == {pre + k for k in have}, "clip schema mismatch"
    te.load_state_dict({k[len(pre):]: v for k, v in csd.items()}, strict=False)
    pd = PIPE["dino"]
    dino = Dinov2Model(Dinov2Config(hidden_size=pd["hidden"], num_hidden_layers=pd["layers"], num_attention_heads=pd["heads"],
                                    image_size=14 * pd["grid"], patch_size=pd["patch"], mlp_ratio=pd["mlp_ratio"])).eval()
    assert set(dsd.keys()) == set(dino.state_dict().keys()), "dinov2 schema mismatch"
    dino.load_state_dict(dsd, strict=True)
    # facebook/dinov2-* preprocessor_config.json values (external knowledge, like the ViT-L sizes): what AutoImageProcessor resolves to
    proc = BitImageProcessor(do_resize=True, size={"shortest_edge": 256}, resample=3, do_center_crop=True,
                             crop_size={"height": 224, "width": 224}, do_rescale=True, rescale_factor=1 / 255, do_normalize=True,
                             image_mean=[0.485, 0.456, 0.406], image_std=[0.229, 0.224, 0.225], do_convert_rgb=True)
    return unet, blob, vae, te, proc, dino


def golden_pipeline_call():
    """The REFERENCE pipeline's own `__call__` (pipe:743-1166) end to end on tiny components: PIL images + prompt strings in, latents
    (and one decoded image) out - tokenizer stand-in, CLIP, VAE encode (global-generator posterior samples), DINOv2 processor + model,
    rank-1 splat, BlobNet + patched UNet loop, scheduler, VAE decode, VaeImageProcessor.postprocess."""
    from PIL import Image
    from tests.common import FakeTokenizer, pipeline_cases
    unet, blob, vae, te, proc, dino = _tiny_pipeline_components()
    rng = np.random.Generator(np.random.PCG64(3))
    # smooth-ish images (random low-res blocks upsampled) so that resize filters matter but nothing saturates
    def img(h, w):
        lo = rng.integers(0, 256, (h // 8, w // 8, 3)).astype(np.uint8)
        return np.kron(lo, np.ones((8, 8, 1), np.uint8)) // 2 + rng.integers(0, 128, (h, w, 3)).astype(np.uint8)
    out = {"fg": img(64, 64), "bg": img(64, 64)}
    ell = [[40.0, 42.0], [20.0, 30.0], 25.0]
    mean, cov = ref_inf.get_gs_from_ellipse(ell)
    nm, nc = ref_inf.normalize_gs(mean, cov, 64, 64)
    gs = splat_features(**ref_inf.get_blob_dict_from_norm_gs(nm, nc), score_size=(8, 8), return_d_score=True)   # [1,2,8,8] f64
    out["gs_score"] = gs.numpy()
    # image-processor pins (host code on our side): DINOv2 preprocessing of non-square images, VAE preprocessing with a resize
    from diffusers.image_processor import VaeImageProcessor
    odd = Image.fromarray(img(72, 104))
    out["odd"] = np.array(odd)
    out["odd_dino_pixels"] = proc.preprocess(images=odd, do_resize=True, return_tensors="pt", do_convert_rgb=True).pixel_values.numpy()
    out["odd_vae_pixels"] = VaeImageProcessor(vae_scale_factor=8, do_convert_rgb=True).preprocess(odd, height=64, width=96).numpy()
    for name, kw in pipeline_cases().items():
        kw = dict(kw)
        sch = (UniPCMultistepScheduler(**SD_SCHED) if kw.pop("scheduler") == "unipc"
               else DDIMScheduler(**SD_SCHED, clip_sample=False, set_alpha_to_one=False))
        pipe = StableDiffusionBlobNetPipeline(vae=vae, unet=unet, tokenizer=FakeTokenizer(), text_encoder=te, blobnet=blob,
                                              scheduler=sch, safety_checker=None, dinov2_processor=proc, dinov2=dino,
                                              requires_safety_checker=False)
        pipe.set_progress_bar_config(disable=True)
        # record what the reference's own front ends hand to its loop (the LOOP-ENTRY tensors): prompt embeddings, image latents in
        # call order (fg, then bg), DINOv2 feature - so that the GPU test can bound the front ends and the loop separately
        entry = {"lat": []}

        def tap(fn, key):
            def wrapped(*a, **k_):
                r_ = fn(*a, **k_)
                if key == "lat":
                    entry["lat"].append(r_.detach().clone())
                else:
                    entry[key] = r_
                return r_
            return wrapped
        pipe.encode_prompt = tap(pipe.encode_prompt, "prompt")
        pipe.encode_latents = tap(pipe.encode_latents, "lat")
        pipe.encode_image_dinov2 = tap(pipe.encode_image_dinov2, "dino")
        seed, rng_seed = kw.pop("seed"), kw.pop("rng_seed")
        common = dict(fg_image=Image.fromarray(out["fg"]), bg_image=Image.fromarray(out["bg"]), gs_score=gs, height=64, width=64, **kw)
        torch.manual_seed(rng_seed)           # the VAE posterior samples come from the GLOBAL generator (pipe:304)
        r = pipe(generator=torch.Generator().manual_seed(seed), output_type="latent", **common)
        out[f"{name}_latents"] = r.images.numpy()
        pe, ne = entry["prompt"]
        out[f"{name}_entry_prompt_embeds"] = pe.numpy()
        if ne is not None:
            out[f"{name}_entry_negative_prompt_embeds"] = ne.numpy()
        out[f"{name}_entry_fg_latents"] = entry["lat"][0][:1].numpy()
        out[f"{name}_entry_bg_latents"] = entry["lat"][1][:1].numpy()
        out[f"{name}_entry_dino"] = entry["dino"].numpy()
        if name == "unipc":
            torch.manual_seed(rng_seed)
            r = pipe(generator=torch.Generator().manual_seed(seed), output_type="np", **common)
            out[f"{name}_image_np"] = np.asarray(r.images)
        print(f"pipeline __call__ {name}: latents std {out[f'{name}_latents'].std():.4f}")
    np.savez_compressed(os.path.join(OUT, "pipeline_call.npz"), **out)


def golden_pipeline_call_eta():
    """The reference's own `__call__` (pipe:743-1166) with DDIM, eta = 1.0 and a CPU `generator`: the generator draws the start latents
    (pipe:438-453), then every scheduler step's variance noise (pipe:313-327, 1102).  Case = `ddim_neg2` of pipeline_call.npz (two
    prompts, negative prompts) with its own seeds; the images and scores are those of pipeline_call.npz.  Stores the final latents,
    the noise tapped from scheduler.step and the loop-entry tensors."""
    from PIL import Image
    from tests.common import FakeTokenizer, pipeline_cases
    unet, blob, vae, te, proc, dino = _tiny_pipeline_components()
    base = np.load(os.path.join(OUT, "pipeline_call.npz"))
    kw = dict(pipeline_cases()["ddim_neg2"], seed=2024, rng_seed=21)
    kw.pop("scheduler")
    sch = DDIMScheduler(**SD_SCHED, clip_sample=False, set_alpha_to_one=False)
    pipe = StableDiffusionBlobNetPipeline(vae=vae, unet=unet, tokenizer=FakeTokenizer(), text_encoder=te, blobnet=blob, scheduler=sch,
                                          safety_checker=None, dinov2_processor=proc, dinov2=dino, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    entry = {"lat": []}

    def tap(fn, key):
        def wrapped(*a, **k_):
            r_ = fn(*a, **k_)
            if key == "lat":
                entry["lat"].append(r_.detach().clone())
            else:
                entry[key] = r_
            return r_
        return wrapped
    pipe.encode_prompt = tap(pipe.encode_prompt, "prompt")
    pipe.encode_latents = tap(pipe.encode_latents, "lat")
    pipe.encode_image_dinov2 = tap(pipe.encode_image_dinov2, "dino")
    seed, rng_seed = kw.pop("seed"), kw.pop("rng_seed")
    out = {"seed": np.array(seed), "rng_seed": np.array(rng_seed), "eta": np.array(1.0)}
    torch.manual_seed(rng_seed)
    with _TapNoise() as noise:
        r = pipe(fg_image=Image.fromarray(base["fg"]), bg_image=Image.fromarray(base["bg"]), gs_score=torch.from_numpy(base["gs_score"]),
                 height=64, width=64, eta=1.0, generator=torch.Generator().manual_seed(seed), output_type="latent", **kw)
    assert len(noise.drawn) == kw["num_inference_steps"]
    out["latents"] = r.images.numpy()
    out["noise"] = torch.stack(noise.drawn).numpy()
    pe, ne = entry["prompt"]
    out["entry_prompt_embeds"], out["entry_negative_prompt_embeds"] = pe.numpy(), ne.numpy()
    out["entry_fg_latents"] = entry["lat"][0][:1].numpy()
    out["entry_bg_latents"] = entry["lat"][1][:1].numpy()
    out["entry_dino"] = entry["dino"].numpy()
    np.savez_compressed(os.path.join(OUT, "pipeline_call_eta.npz"), **out)
    print(f"pipeline __call__ eta=1: latents std {out['latents'].std():.4f}, noise {out['noise'].shape}")


def golden_blocks():
    """single diffusers blocks at SD-1.5 widths on small feature maps (resnet.py:320-373, transformer_2d.py:479-527,
    upsampling.py:141-184, downsampling.py:132-149, embeddings.py:27-78 + 576-588).  Only the OUTPUTS are stored (fp32); weights and
    inputs are regenerated from seeds on both sides (tests/common.py block_weights / block_inputs)."""
    from diffusers.models.resnet import ResnetBlock2D
    from diffusers.models.transformers.transformer_2d import Transformer2DModel
    from diffusers.models.upsampling import Upsample2D
    from diffusers.models.downsampling import Downsample2D
    from diffusers.models.embeddings import Timesteps, TimestepEmbedding
    from tests.common import BLOCK_CASES, BLOCK_TIMESTEPS, block_inputs, block_weights
    out = {}
    for name, (kind, p) in BLOCK_CASES.items():
        x, temb, ctx = block_inputs(name)
        if kind == "resnet":       # as the UNet blocks build it (unet_2d_blocks.py: eps=resnet_eps=1e-5, groups=32, temb 1280)
            m = ResnetBlock2D(in_channels=p["cin"], out_channels=p["cout"], temb_channels=1280, eps=1e-5, groups=32)
        elif kind == "transformer":
            m = Transformer2DModel(num_attention_heads=p["heads"], attention_head_dim=p["C"] // p["heads"], in_channels=p["C"],
                                   num_layers=1, cross_attention_dim=p["ctx"], norm_num_groups=32)
        elif kind == "upsample":
            m = Upsample2D(p["C"], use_conv=True, out_channels=p["C"])
        else:
            m = Downsample2D(p["C"], use_conv=True, out_channels=p["C"], padding=1, name="op")
        m.eval()
        sd = block_weights(name)
        assert set(sd.keys()) == set(m.state_dict().keys()), (name, set(sd.keys()) ^ set(m.state_dict().keys()))
        m.load_state_dict(sd, strict=True)
        if kind == "resnet":
            y = m(x, temb)
        elif kind == "transformer":
            y = m(x, encoder_hidden_states=ctx, return_dict=False)[0]
        elif kind == "upsample":
            y = m(x, output_size=p["size"])
        else:
            y = m(x)
        sub = p.get("sub", 1)
        out[name] = y.numpy().astype(np.float32)[:, :, ::sub, ::sub]
        print(f"block {name}: out {tuple(y.shape)} std {float(y.std()):.4f} stored {out[name].shape}")
    proj, emb = Timesteps(320, True, 0), TimestepEmbedding(320, 1280).eval()
    emb.load_state_dict(block_weights("time"), strict=True)
    t = torch.tensor(BLOCK_TIMESTEPS)
    out["time_sinusoid"] = proj(t).numpy()
    out["time_emb"] = emb(proj(t)).numpy()
    np.savez_compressed(os.path.join(OUT, "blocks.npz"), **out)


def golden_ip_adapter():
    """tests/golden/unet_tiny_ip.npz: the tiny UNet of build_tiny() after the reference's `unet._load_ip_adapter_weights` (D/loaders/
    unet.py:823-853) with the synthetic base adapters of tests/ip_adapter_common.py tiny_ip_adapter, called with
    added_cond_kwargs={"image_embeds": [...]} and BlobNet-style residual stand-ins (freeu_residuals).  Per case (IP_UNET_CASES: one
    adapter with one image on the wide canvas, two adapters with two and one images on the square one): `eps` at the case's scales,
    `eps_off` with every processor scale 0 - asserted bit-equal to the adapter-less UNet - and `eps_other_scale` at IP_OTHER_FACTOR times
    the scales; plus the (key id -> processor name, shape) list the reference's loader walks.  The variants must lie at least 10 times
    the GPU bar (1e-2 of eps' scale, tests/test_freeu_gpu.py) apart."""
    from diffusers.models.attention_processor import IPAdapterAttnProcessor2_0
    from tests.ip_adapter_common import (IP_GEOMETRIES, IP_OTHER_FACTOR, IP_RES_SCALE, IP_UNET_CASES, IP_UNET_SCALES, ip_unet_inputs,
                                         tiny_ip_adapter)
    out, t = {"timestep": np.array(981), "res_scale": np.array(IP_RES_SCALE), "other_factor": np.array(IP_OTHER_FACTOR)}, torch.tensor(981)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    for case, (geo, images) in IP_UNET_CASES.items():
        B, H, W = IP_GEOMETRIES[geo]
        x_u, ehs, seed, embeds = ip_unet_inputs(case)
        down, mid, up = _freeu_residual_shapes(H, W)
        mk = lambda i, s: g(seed + i, B, *s) * IP_RES_SCALE
        down, mid, up = [mk(i, s) for i, s in enumerate(down)], mk(100, mid), [mk(200 + i, s) for i, s in enumerate(up)]
        res = lambda: dict(down_block_add_samples=[r.clone() for r in down], mid_block_add_sample=mid.clone(),
                           up_block_add_samples=[r.clone() for r in up])
        plain, _ = build_tiny()
        with torch.no_grad():
            eps_plain = plain(x_u, t, encoder_hidden_states=ehs, return_dict=False, **res())[0].numpy()
        unet, _ = build_tiny()
        unet._load_ip_adapter_weights([tiny_ip_adapter(i) for i in range(len(images))], low_cpu_mem_usage=False)
        assert unet.config.encoder_hid_dim_type == "ip_image_proj"
        procs = [(n, p) for n, p in unet.attn_processors.items() if isinstance(p, IPAdapterAttnProcessor2_0)]
        assert len(procs) == 16 and all(p.scale == [1.0] * len(images) for _, p in procs)

        def run(factor):
            for _, p in procs:
                p.scale = [factor * s_ for s_ in IP_UNET_SCALES[case]]
            with torch.no_grad():
                return unet(x_u, t, encoder_hidden_states=ehs, added_cond_kwargs={"image_embeds": embeds}, return_dict=False, **res())[0].numpy()
        eps, eps_off, eps_other = run(1.0), run(0.0), run(IP_OTHER_FACTOR)
        assert np.array_equal(eps_off, eps_plain), "scale 0 is the adapter-less UNet, bit for bit"
        gaps = dict(on_off=rel(eps, eps_off) / 1e-2, on_other=rel(eps, eps_other) / 1e-2, other_off=rel(eps_other, eps_off) / 1e-2)
        print(f"ip-adapter UNet {case}: eps std {eps.std():.4f}, variants apart by {gaps} bars")
        assert min(gaps.values()) >= 10.0, (case, gaps)
        out.update({f"{case}_eps": eps, f"{case}_eps_off": eps_off, f"{case}_eps_other_scale": eps_other})
        out["key_names"] = np.array([n for n, _ in procs])
        out["key_ids"] = np.array([1 + 2 * j for j in range(len(procs))])
        out["key_shapes"] = np.array([tuple(p.to_k_ip[0].weight.shape) for _, p in procs])
    np.savez_compressed(os.path.join(OUT, "unet_tiny_ip.npz"), **out)
    print("unet_tiny_ip.npz: %.1f KB" % (os.path.getsize(os.path.join(OUT, "unet_tiny_ip.npz")) / 1024))


def golden_pipeline_call_ip():
    """tests/golden/pipeline_call_ip.npz: the reference's own `__call__` (pipe:743-1166) with one synthetic base IP-Adapter loaded into its
    UNet (`unet._load_ip_adapter_weights`, tiny_ip_adapter(0)) and `ip_adapter_image_embeds` given.  The reference class calls
    `self.prepare_ip_adapter_image_embeds` (pipe:925) without having copied it, so the vendored function of D/pipelines/stable_diffusion/
    pipeline_stable_diffusion.py:508 is bound onto the pipeline object (types.MethodType); with that the bound call runs.  DDIM, 3 steps,
    the case `ddim_neg2` of pipeline_call.npz with seeds of its own.  Stores the final latents at IP_CALL_SCALE (`latents`), at
    IP_CALL_SCALE_OTHER (`latents_other`), with the adapter-less UNet (`latents_off`: a pipeline that never loaded one, what unload
    gives back), the per-processor scale lists the reference ends up with for a float, a list and a dict argument, and the embeddings.
    The variants lie at least 10 times the GPU bar (1e-2 of the latents' scale) apart."""
    from PIL import Image
    from diffusers.loaders.ip_adapter import IPAdapterMixin
    from diffusers.models.attention_processor import IPAdapterAttnProcessor2_0
    from diffusers.pipelines.stable_diffusion.pipeline_stable_diffusion import StableDiffusionPipeline
    from tests.common import FakeTokenizer, pipeline_cases
    from tests.ip_adapter_common import IP_CALL_SCALE, IP_CALL_SCALE_DICT, IP_CALL_SCALE_OTHER, ip_call_embeds, tiny_ip_adapter
    base = np.load(os.path.join(OUT, "pipeline_call.npz"))
    kw = dict(pipeline_cases()["ddim_neg2"], seed=2041, rng_seed=41)
    kw.pop("scheduler")
    kw["num_inference_steps"] = 3
    seed, rng_seed = kw.pop("seed"), kw.pop("rng_seed")
    embeds = ip_call_embeds()

    def make(adapter):
        unet, blob, vae, te, proc, dino = _tiny_pipeline_components()
        if adapter:
            unet._load_ip_adapter_weights([tiny_ip_adapter(0)], low_cpu_mem_usage=False)
        sch = DDIMScheduler(**SD_SCHED, clip_sample=False, set_alpha_to_one=False)
        pipe = StableDiffusionBlobNetPipeline(vae=vae, unet=unet, tokenizer=FakeTokenizer(), text_encoder=te, blobnet=blob, scheduler=sch,
                                              safety_checker=None, dinov2_processor=proc, dinov2=dino, requires_safety_checker=False)
        pipe.set_progress_bar_config(disable=True)
        assert not hasattr(pipe, "prepare_ip_adapter_image_embeds")
        pipe.prepare_ip_adapter_image_embeds = types.MethodType(StableDiffusionPipeline.prepare_ip_adapter_image_embeds, pipe)
        return pipe

    def call(pipe, **extra):
        torch.manual_seed(rng_seed)
        return pipe(fg_image=Image.fromarray(base["fg"]), bg_image=Image.fromarray(base["bg"]), gs_score=torch.from_numpy(base["gs_score"]),
                    height=64, width=64, generator=torch.Generator().manual_seed(seed), output_type="latent", **extra, **kw).images.numpy()
    pipe = make(True)
    procs = [p_ for p_ in pipe.unet.attn_processors.values() if isinstance(p_, IPAdapterAttnProcessor2_0)]
    lists = {}
    for tag, arg in (("float", IP_CALL_SCALE), ("list", [IP_CALL_SCALE_OTHER]), ("dict", IP_CALL_SCALE_DICT)):
        IPAdapterMixin.set_ip_adapter_scale(pipe, arg)
        lists[tag] = np.array([float(p_.scale[0]) for p_ in procs])
    out = {"seed": np.array(seed), "rng_seed": np.array(rng_seed), "num_inference_steps": np.array(kw["num_inference_steps"]),
           "embeds": embeds.numpy(), **{f"scales_{k}": v for k, v in lists.items()}}
    IPAdapterMixin.set_ip_adapter_scale(pipe, IP_CALL_SCALE)
    out["latents"] = call(pipe, ip_adapter_image_embeds=[embeds])
    IPAdapterMixin.set_ip_adapter_scale(pipe, IP_CALL_SCALE_OTHER)
    out["latents_other"] = call(pipe, ip_adapter_image_embeds=[embeds])
    out["latents_off"] = call(make(False))
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    gaps = (rel(out["latents"], out["latents_off"]), rel(out["latents_other"], out["latents"]), rel(out["latents_other"], out["latents_off"]))
    print("pipeline __call__ ip-adapter: latents std %.4f; on vs off %.3f, other vs on %.3f, other vs off %.3f (max-abs / scale)" %
          ((out["latents"].std(),) + gaps))
    assert min(gaps) >= 10 * 1e-2, gaps
    np.savez_compressed(os.path.join(OUT, "pipeline_call_ip.npz"), **out)
    print("pipeline_call_ip.npz: %.1f KB" % (os.path.getsize(os.path.join(OUT, "pipeline_call_ip.npz")) / 1024))


def golden_blocks_ip():
    """tests/golden/blocks_ip.npz: one Transformer2DModel at 320, 640 and 1280 channels with IPAdapterAttnProcessor2_0 on attn2
    (D/models/attention_processor.py:3656-3883), called with encoder_hidden_states=(text, [tokens per adapter]) - what the UNet hands
    its blocks once encoder_hid_proj has projected the image embeddings.  Per case (tests/ip_adapter_common.py IP_BLOCK_CASES): `<name>`
    at the case's scales, `<name>_off` with every scale 0 (the reference skips the adapter) and `<name>_other` at half the scales.
    Outputs only (fp32, every `sub`-th pixel); weights, inputs and tokens come from seeds on both sides.  The variants must lie at least
    10 times the GPU bar of tests/test_blocks_gpu.py (1e-2 of the output's scale) apart, or the test could not tell them apart."""
    from diffusers.models.attention_processor import IPAdapterAttnProcessor2_0
    from diffusers.models.transformers.transformer_2d import Transformer2DModel
    from tests.ip_adapter_common import IP_BLOCK_CASES, IP_BLOCK_SCALES, ip_block_inputs, ip_block_weights
    out = {}
    for name, p in IP_BLOCK_CASES.items():
        x, ctx, tokens = ip_block_inputs(name)
        m = Transformer2DModel(num_attention_heads=p["heads"], attention_head_dim=p["C"] // p["heads"], in_channels=p["C"], num_layers=1,
                               cross_attention_dim=p["ctx"], norm_num_groups=32).eval()
        sd, ip = ip_block_weights(name)
        m.load_state_dict(sd, strict=True)
        proc = IPAdapterAttnProcessor2_0(p["C"], p["ctx"], num_tokens=list(p["tokens"]), scale=list(IP_BLOCK_SCALES[name]))
        for i, (wk, wv) in enumerate(ip):
            proc.to_k_ip[i].weight.data.copy_(wk)
            proc.to_v_ip[i].weight.data.copy_(wv)
        m.transformer_blocks[0].attn2.set_processor(proc)
        sub, res = p["sub"], {}
        for tag, f in (("", 1.0), ("_off", 0.0), ("_other", 0.5)):
            proc.scale = [f * s_ for s_ in IP_BLOCK_SCALES[name]]
            with torch.no_grad():
                y = m(x, encoder_hidden_states=(ctx, tokens), return_dict=False)[0]
            res[tag] = out[name + tag] = y.numpy().astype(np.float32)[:, :, ::sub, ::sub]
        bar = 1e-2 * np.abs(res[""]).max()
        gaps = {a + "/" + b: float(np.abs(res[a] - res[b]).max() / bar) for a, b in (("", "_off"), ("", "_other"), ("_other", "_off"))}
        print(f"block {name}: out std {res[''].std():.4f}, variants apart by {gaps} bars")
        assert min(gaps.values()) >= 10.0, (name, gaps)
    np.savez_compressed(os.path.join(OUT, "blocks_ip.npz"), **out)


def golden_clip_vision():
    """tests/golden/clip_vision_tiny.npz: transformers' CLIPVisionModelWithProjection at the two random tiny configurations of
    tests/clip_vision_common.py CLIP_VISION_CONFIGS, the seeded state dict loaded after its key set is asserted equal to the model's (`position_ids` aside: the key names are the installed ones), batch 2:
    `<name>_image_embeds`, `<name>_hidden` = hidden_states[-2], and both again for an all-zero input (`_zero`: what the reference's
    encode_image feeds the negative branch of an IP-Adapter Plus).  Outputs only."""
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    from tests.clip_vision_common import CLIP_VISION_CONFIGS, clip_vision_pixels, clip_vision_weights
    out = {}
    for name, c in CLIP_VISION_CONFIGS.items():
        model = CLIPVisionModelWithProjection(CLIPVisionConfig(**c)).eval()
        have = {k for k in model.state_dict() if not k.endswith("position_ids")}
        sd = clip_vision_weights(name, prefix="vision_model." if any(k.startswith("vision_model.") for k in have) else "")
        assert set(sd) == have, (sorted(set(sd) ^ have))
        model.load_state_dict(sd, strict=False)
        px = clip_vision_pixels(name)
        for tag, x in (("", px), ("_zero", torch.zeros_like(px))):
            with torch.no_grad():
                r = model(pixel_values=x, output_hidden_states=True)
            assert len(r.hidden_states) == c["num_hidden_layers"] + 1
            out[f"{name}_image_embeds{tag}"], out[f"{name}_hidden{tag}"] = r.image_embeds.numpy(), r.hidden_states[-2].numpy()
        gap = float(np.abs(out[f"{name}_hidden"] - out[f"{name}_hidden_zero"]).max() / np.abs(out[f"{name}_hidden"]).max()) / 1e-2
        print(f"clip vision {name}: image_embeds std {out[f'{name}_image_embeds'].std():.3f}, hidden std {out[f'{name}_hidden'].std():.3f}, "
              f"seeded vs zero input {gap:.0f} bars")
        assert gap >= 10.0, gap
    np.savez_compressed(os.path.join(OUT, "clip_vision_tiny.npz"), **out)
    print("clip_vision_tiny.npz: %.1f KB" % (os.path.getsize(os.path.join(OUT, "clip_vision_tiny.npz")) / 1024))


def golden_pipeline_call_ip_image():
    """tests/golden/pipeline_call_ip_image.npz: the reference's own `__call__` with `ip_adapter_image=<PIL image>`.  The tiny CLIP tower
    "a" of tests/clip_vision_common.py (transformers' CLIPVisionModelWithProjection, seeded weights) is set as `image_encoder`;
    `clip_processor` and `feature_extractor` (CLIPImageProcessor at the tower's 42 pixels) are bound on the object because the class
    forgets them, and `prepare_ip_adapter_image_embeds` is bound as golden_pipeline_call_ip does.  DDIM, 3 steps, the case `ddim_neg2`
    of pipeline_call.npz; the Plus adapter (tiny_plus_adapter "q16") and the base adapter (tiny_ip_adapter(0)) in turn.  Stores the final
    latents `<kind>_latents` for image A, `<kind>_latents_b` for image B and `latents_off` of a pipeline without an adapter; the variants
    lie at least 10 GPU bars (1e-2 of the latents' scale) apart."""
    from PIL import Image
    from diffusers.pipelines.stable_diffusion.pipeline_stable_diffusion import StableDiffusionPipeline
    from transformers import CLIPImageProcessor, CLIPVisionConfig, CLIPVisionModelWithProjection
    from tests.clip_vision_common import (CLIP_VISION_CONFIGS, IP_IMAGE_CALL_IMAGES, IP_IMAGE_CALL_SEEDS, clip_processor_image,
                                          clip_vision_weights, tiny_plus_adapter)
    from tests.common import FakeTokenizer, pipeline_cases
    from tests.ip_adapter_common import tiny_ip_adapter
    base = np.load(os.path.join(OUT, "pipeline_call.npz"))
    kw = dict(pipeline_cases()["ddim_neg2"])
    for k in ("scheduler", "seed", "rng_seed"):
        kw.pop(k)
    kw["num_inference_steps"] = 3
    seed, rng_seed = IP_IMAGE_CALL_SEEDS
    c = CLIP_VISION_CONFIGS["a"]
    tower = CLIPVisionModelWithProjection(CLIPVisionConfig(**c)).eval()
    have = {k for k in tower.state_dict() if not k.endswith("position_ids")}
    sd = clip_vision_weights("a", prefix="vision_model." if any(k.startswith("vision_model.") for k in have) else "")
    assert set(sd) == have
    tower.load_state_dict(sd, strict=False)
    images = {k: Image.fromarray(clip_processor_image(v)) for k, v in IP_IMAGE_CALL_IMAGES.items()}

    def make(adapter):
        unet, blob, vae, te, proc, dino = _tiny_pipeline_components()
        if adapter is not None:
            unet._load_ip_adapter_weights([adapter], low_cpu_mem_usage=False)
        sch = DDIMScheduler(**SD_SCHED, clip_sample=False, set_alpha_to_one=False)
        pipe = StableDiffusionBlobNetPipeline(vae=vae, unet=unet, tokenizer=FakeTokenizer(), text_encoder=te, blobnet=blob, scheduler=sch,
                                              safety_checker=None, dinov2_processor=proc, dinov2=dino, requires_safety_checker=False)
        pipe.set_progress_bar_config(disable=True)
        pipe.image_encoder = tower
        pipe.clip_processor = pipe.feature_extractor = CLIPImageProcessor(size=c["image_size"], crop_size=c["image_size"])
        pipe.prepare_ip_adapter_image_embeds = types.MethodType(StableDiffusionPipeline.prepare_ip_adapter_image_embeds, pipe)
        return pipe

    def call(pipe, **extra):
        torch.manual_seed(rng_seed)
        return pipe(fg_image=Image.fromarray(base["fg"]), bg_image=Image.fromarray(base["bg"]), gs_score=torch.from_numpy(base["gs_score"]),
                    height=64, width=64, generator=torch.Generator().manual_seed(seed), output_type="latent", **extra, **kw).images.numpy()
    out = {"seed": np.array(seed), "rng_seed": np.array(rng_seed), "num_inference_steps": np.array(3), "latents_off": call(make(None))}
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    for kind, adapter in (("plus", tiny_plus_adapter("q16")), ("base", tiny_ip_adapter(0))):
        pipe = make(adapter)
        out[f"{kind}_latents"] = call(pipe, ip_adapter_image=images["a"])
        out[f"{kind}_latents_b"] = call(pipe, ip_adapter_image=images["b"])
        gaps = (rel(out[f"{kind}_latents"], out["latents_off"]), rel(out[f"{kind}_latents_b"], out[f"{kind}_latents"]),
                rel(out[f"{kind}_latents_b"], out["latents_off"]))
        print("pipeline __call__ ip image %s: latents std %.4f; A vs off %.3f, B vs A %.3f, B vs off %.3f (max-abs / scale)" %
              ((kind, out[f"{kind}_latents"].std()) + gaps))
        assert min(gaps) >= 10 * 1e-2, (kind, gaps)
    np.savez_compressed(os.path.join(OUT, "pipeline_call_ip_image.npz"), **out)
    print("pipeline_call_ip_image.npz: %.1f KB" % (os.path.getsize(os.path.join(OUT, "pipeline_call_ip_image.npz")) / 1024))


def golden_clip_processor():
    """tests/golden/clip_processor.npz: the installed transformers CLIPImageProcessor - without torchvision it falls back to its Pillow
    backend, the one to pin - on the seeded images of tests/clip_vision_common.py: `<image>_<size>` = pixel_values [3][size][size] at
    size = crop = 224 and 56."""
    from PIL import Image
    from transformers import CLIPImageProcessor
    from tests.clip_vision_common import CLIP_PROCESSOR_IMAGES, CLIP_PROCESSOR_SIZES, clip_processor_image
    out = {}
    for size in CLIP_PROCESSOR_SIZES:
        proc = CLIPImageProcessor(size={"shortest_edge": size}, crop_size={"height": size, "width": size})
        assert "Pil" in type(proc).__name__, type(proc).__name__
        for name in CLIP_PROCESSOR_IMAGES:
            px = proc(images=Image.fromarray(clip_processor_image(name)), return_tensors="pt").pixel_values
            assert tuple(px.shape) == (1, 3, size, size) and px.dtype == torch.float32
            out[f"{name}_{size}"] = px[0].numpy()
    np.savez_compressed(os.path.join(OUT, "clip_processor.npz"), **out)
    print("clip_processor.npz: %.1f KB" % (os.path.getsize(os.path.join(OUT, "clip_processor.npz")) / 1024))


def golden_ip_plus():
    """tests/golden/ip_plus_tiny.npz: IP-Adapter Plus on the tiny UNet of build_tiny().  The synthetic Plus adapters of
    tests/clip_vision_common.py (original key spelling: the reference's loader renames them, D/loaders/unet.py:657-724) go through
    `unet._load_ip_adapter_weights`; stored are
      tokens_<q16|q8>_<one|two>   encoder_hid_proj's IPAdapterPlusImageProjection on hidden states [2][1][10][64] / [2][2][10][64], as
                                  MultiIPAdapterImageProjection lays them out: [2][images * queries][ctx]
      <case>_eps / _eps_off / _eps_other_scale   the UNet of PLUS_UNET_CASES (one image, two images = 32 tokens, a Plus and a base adapter
                                  together) as golden_ip_adapter stores its cases; eps_off is asserted bit-equal to the adapter-less UNet.
    Variants a test must tell apart (on / off / other scale, one / two images' tokens) lie at least 10 GPU bars (1e-2 of the scale) apart."""
    from diffusers.models.attention_processor import IPAdapterAttnProcessor2_0
    from diffusers.models.embeddings import IPAdapterPlusImageProjection
    from tests.clip_vision_common import (PLUS_QUERIES, PLUS_TOKEN_SHAPES, PLUS_UNET_CASES, PLUS_UNET_SCALES, plus_hidden, plus_unet_adapters,
                                          plus_unet_inputs, tiny_plus_adapter)
    from tests.ip_adapter_common import IP_GEOMETRIES, IP_OTHER_FACTOR, IP_RES_SCALE
    out, t = {"timestep": np.array(981), "res_scale": np.array(IP_RES_SCALE), "other_factor": np.array(IP_OTHER_FACTOR)}, torch.tensor(981)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    for kind in PLUS_QUERIES:
        unet, _ = build_tiny()
        unet._load_ip_adapter_weights([tiny_plus_adapter(kind)], low_cpu_mem_usage=False)
        proj = unet.encoder_hid_proj.image_projection_layers[0]
        assert isinstance(proj, IPAdapterPlusImageProjection) and proj.latents.shape[1] == PLUS_QUERIES[kind] and len(proj.layers) == 4
        for name in PLUS_TOKEN_SHAPES:
            with torch.no_grad():
                tok = unet.encoder_hid_proj([plus_hidden(name)])[0]              # [2][images][queries][ctx]
            tok = tok.reshape(tok.shape[0], -1, tok.shape[-1])
            assert tok.shape[:2] ==(2, PLUS_TOKEN_SHAPES[name][1] * PLUS_QUERIES[kind])
            out[f"tokens_{kind}_{name}"] = tok.numpy()
        gap = rel(out[f"tokens_{kind}_two"][:, :PLUS_QUERIES[kind]], out[f"tokens_{kind}_one"]) / 1e-2
        print(f"ip-adapter plus {kind}: tokens std {out[f'tokens_{kind}_one'].std():.3f}, first image of `two` vs `one` {gap:.0f} bars")
        assert gap >= 10.0, gap
    for case, (geo, adapters) in PLUS_UNET_CASES.items():
        B, H, W = IP_GEOMETRIES[geo]
        x_u, ehs, seed, ins = plus_unet_inputs(case)
        down, mid, up = _freeu_residual_shapes(H, W)
        mk = lambda i, s: g(seed + i, B, *s) * IP_RES_SCALE
        down, mid, up = [mk(i, s) for i, s in enumerate(down)], mk(100, mid), [mk(200 + i, s) for i, s in enumerate(up)]
        res = lambda: dict(down_block_add_samples=[r.clone() for r in down], mid_block_add_sample=mid.clone(),
                           up_block_add_samples=[r.clone() for r in up])
        plain, _ = build_tiny()
        with torch.no_grad():
            eps_plain = plain(x_u, t, encoder_hidden_states=ehs, return_dict=False, **res())[0].numpy()
        unet, _ = build_tiny()
        unet._load_ip_adapter_weights(plus_unet_adapters(case), low_cpu_mem_usage=False)
        procs = [p for p in unet.attn_processors.values() if isinstance(p, IPAdapterAttnProcessor2_0)]
        assert len(procs) == 16

        def run(factor):
            for p in procs:
                p.scale = [factor * s_ for s_ in PLUS_UNET_SCALES[case]]
            with torch.no_grad():
                return unet(x_u, t, encoder_hidden_states=ehs, added_cond_kwargs={"image_embeds": ins}, return_dict=False, **res())[0].numpy()
        eps, eps_off, eps_other = run(1.0), run(0.0), run(IP_OTHER_FACTOR)
        assert np.array_equal(eps_off, eps_plain), "scale 0 is the adapter-less UNet, bit for bit"
        gaps = dict(on_off=rel(eps, eps_off) / 1e-2, on_other=rel(eps, eps_other) / 1e-2, other_off=rel(eps_other, eps_off) / 1e-2)
        print(f"ip-adapter plus UNet {case}: eps std {eps.std():.4f}, variants apart by {gaps} bars")
        assert min(gaps.values()) >= 10.0, (case, gaps)
        out.update({f"{case}_eps": eps, f"{case}_eps_off": eps_off, f"{case}_eps_other_scale": eps_other})
    np.savez_compressed(os.path.join(OUT, "ip_plus_tiny.npz"), **out)
    print("ip_plus_tiny.npz: %.1f KB" % (os.path.getsize(os.path.join(OUT, "ip_plus_tiny.npz")) / 1024))


def golden_overlay():
    """The vendored `VaeImageProcessor`'s own get_crop_region, apply_overlay, blur and resize("fill" | "crop") on the cases of
    tests/overlay_common.py: ties blobctrl_amd.overlay's restatement to the reference, not only to Pillow."""
    from PIL import Image
    from diffusers.image_processor import VaeImageProcessor
    from tests import overlay_common as oc
    proc, out = VaeImageProcessor(), {}
    for name, ((H, W), box, (width, height), pad) in oc.CROP_CASES.items():
        out[f"crop_{name}"] = np.array(proc.get_crop_region(Image.fromarray(oc.box_mask(H, W, *box)), width, height, pad=pad), dtype=np.int64)
    for name in oc.OVERLAY_CASES:
        mask, init, image, crop = oc.overlay_inputs(name)
        out[f"overlay_{name}"] = np.array(proc.apply_overlay(Image.fromarray(mask), Image.fromarray(init), Image.fromarray(image), crop))
    mask, init, image = oc.overlay_resized_inputs()
    out["overlay_resized"] = np.array(proc.apply_overlay(Image.fromarray(mask), Image.fromarray(init), Image.fromarray(image)))
    for name, ((H, W), (width, height), seed) in oc.RESIZE_CASES.items():
        img = Image.fromarray(oc.rgb_image(H, W, seed))
        out[f"fill_{name}"] = np.array(proc.resize(img, height, width, resize_mode="fill"))
        out[f"fit_{name}"] = np.array(proc.resize(img, height, width, resize_mode="crop"))
    for name, ((H, W), factor, seed) in oc.BLUR_GOLDEN.items():
        out[f"blur_{name}"] = np.array(proc.blur(Image.fromarray(oc.blob_mask(H, W, seed, hard="hard" in name)), factor))
    np.savez_compressed(oc.GOLDEN, **out)
    print("overlay.npz: %.1f KB, %d arrays" % (os.path.getsize(oc.GOLDEN) / 1024, len(out)))


def golden_ip_mask_downsample():
    """tests/golden/ip_mask_downsample.npz: IPAdapterMaskProcessor.downsample (D/image_processor.py:969-1029) of the two 0 / 1 masks of
    tests/ip_masks_common.py downsample_masks for every (H, W, rows) of DOWNSAMPLE_CASES, batch 1, one value per row (value_embed_dim 1):
    `<H>x<W>_<rows>` fp32 [2][rows], and `<H>x<W>_<rows>_warned` whether the reference warned about the aspect ratio.  The grids must be
    those the formula predicts (DOWNSAMPLE_GRIDS) and exactly the padded cases warn."""
    import warnings
    from diffusers.image_processor import IPAdapterMaskProcessor
    from tests.ip_masks_common import DOWNSAMPLE_CASES, DOWNSAMPLE_GRIDS, DOWNSAMPLE_PADDED, downsample_masks
    out = {}
    for H, W, rows in DOWNSAMPLE_CASES:
        m = torch.from_numpy(downsample_masks(H, W).astype(np.float32))
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            y = torch.stack([IPAdapterMaskProcessor.downsample(m[i:i + 1], 1, rows, 1)[0, :, 0] for i in range(m.shape[0])]).numpy()
        warned = any(issubclass(c.category, UserWarning) and "aspect ratio" in str(c.message) for c in caught)
        mh, mw = DOWNSAMPLE_GRIDS[(H, W, rows)]
        assert y.shape == (2, rows) and warned == ((H, W, rows) in DOWNSAMPLE_PADDED) == (mh * mw < rows), (H, W, rows, warned)
        assert not y[:, mh * mw:].any() and (mh * mw == rows or y[:, :mh * mw].any())
        print(f"ip mask downsample {H} x {W} -> {rows} rows ({mh} x {mw}): range [{y.min():.3f}, {y.max():.3f}], warned {warned}")
        out[f"{H}x{W}_{rows}"], out[f"{H}x{W}_{rows}_warned"] = y.astype(np.float32), np.array(warned)
    np.savez_compressed(os.path.join(OUT, "ip_mask_downsample.npz"), **out)
    print("ip_mask_downsample.npz: %.1f KB" % (os.path.getsize(os.path.join(OUT, "ip_mask_downsample.npz")) / 1024))


def golden_blocks_ip_masks():
    """tests/golden/blocks_ip_masks.npz: the blocks of golden_blocks_ip called with cross_attention_kwargs={"ip_adapter_masks": [...]}
    (D/models/attention_processor.py:3776-3849), every adapter's tokens handed over as [B][images][4][ctx] and the masks of
    tests/ip_masks_common.py block_masks.  Per case: `<name>_masked`, `<name>_unmasked` (no masks: one softmax over all images) and, where
    an adapter has two images, `<name>_swapped` (their masks exchanged).  The variants must lie at least 10 times the GPU bar of
    tests/test_blocks_gpu.py (1e-2 of the output's scale) apart: otherwise the test could not tell a mask applied to the wrong image, or a
    shared softmax, from the truth."""
    import warnings
    from diffusers.models.attention_processor import IPAdapterAttnProcessor2_0
    from diffusers.models.transformers.transformer_2d import Transformer2DModel
    from tests.ip_adapter_common import IP_BLOCK_CASES, IP_BLOCK_SCALES, ip_block_inputs, ip_block_weights
    from tests.ip_masks_common import block_has_swap, block_masks, images_of, swap_images
    out = {}
    for name, p in IP_BLOCK_CASES.items():
        x, ctx, tokens = ip_block_inputs(name)
        m = Transformer2DModel(num_attention_heads=p["heads"], attention_head_dim=p["C"] // p["heads"], in_channels=p["C"], num_layers=1,
                               cross_attention_dim=p["ctx"], norm_num_groups=32).eval()
        sd, ip = ip_block_weights(name)
        m.load_state_dict(sd, strict=True)
        proc = IPAdapterAttnProcessor2_0(p["C"], p["ctx"], num_tokens=list(p["tokens"]), scale=list(IP_BLOCK_SCALES[name]))
        for i, (wk, wv) in enumerate(ip):
            proc.to_k_ip[i].weight.data.copy_(wk)
            proc.to_v_ip[i].weight.data.copy_(wv)
        m.transformer_blocks[0].attn2.set_processor(proc)
        per_image = [t.reshape(t.shape[0], n, 4, t.shape[2]) for t, n in zip(tokens, images_of(p["tokens"]))]
        masks = block_masks(name)
        sub, res = p["sub"], {}
        variants = [("_masked", per_image, masks), ("_unmasked", tokens, None)] + ([("_swapped", per_image, swap_images(masks))] if block_has_swap(name) else [])
        for tag, toks, mk in variants:
            with torch.no_grad(), warnings.catch_warnings():
                warnings.simplefilter("error")                            # (the masks have the canvas' aspect ratio: nothing is padded)
                y = m(x, encoder_hidden_states=(ctx, toks), return_dict=False,
                      **({} if mk is None else dict(cross_attention_kwargs={"ip_adapter_masks": mk})))[0]
            res[tag] = out[name + tag] = y.numpy().astype(np.float32)[:, :, ::sub, ::sub]
        bar = 1e-2 * np.abs(res["_masked"]).max()
        tags = [t for t, _, _ in variants]
        gaps = {a + "/" + b: float(np.abs(res[a] - res[b]).max() / bar) for i, a in enumerate(tags) for b in tags[i + 1:]}
        print(f"block {name} with masks: out std {res['_masked'].std():.4f}, variants apart by {gaps} bars")
        assert min(gaps.values()) >= 10.0, (name, gaps)
    np.savez_compressed(os.path.join(OUT, "blocks_ip_masks.npz"), **out)
    print("blocks_ip_masks.npz: %.1f KB" % (os.path.getsize(os.path.join(OUT, "blocks_ip_masks.npz")) / 1024))


def golden_unet_ip_masks():
    """tests/golden/unet_tiny_ip_masks.npz: the cases of golden_ip_adapter (same UNet, adapters, inputs and residual stand-ins, the
    case's scales) called with cross_attention_kwargs={"ip_adapter_masks": [...]}, masks at the image resolution
    (tests/ip_masks_common.py unet_masks).  Per case `<case>_eps_masked`, and `<case>_eps_swapped` where an adapter has two images; the
    unmasked `eps` is that of unet_tiny_ip.npz.  The variants lie at least 10 GPU bars (1e-2 of eps' scale) apart."""
    from diffusers.models.attention_processor import IPAdapterAttnProcessor2_0
    from tests.ip_adapter_common import IP_GEOMETRIES, IP_RES_SCALE, IP_UNET_CASES, IP_UNET_SCALES, ip_unet_inputs, tiny_ip_adapter
    from tests.ip_masks_common import swap_images, unet_masks
    base = np.load(os.path.join(OUT, "unet_tiny_ip.npz"))
    out, t = {}, torch.tensor(int(base["timestep"]))
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    for case, (geo, images) in IP_UNET_CASES.items():
        B, H, W = IP_GEOMETRIES[geo]
        x_u, ehs, seed, embeds = ip_unet_inputs(case)
        down, mid, up = _freeu_residual_shapes(H, W)
        mk = lambda i, s: g(seed + i, B, *s) * IP_RES_SCALE
        down, mid, up = [mk(i, s) for i, s in enumerate(down)], mk(100, mid), [mk(200 + i, s) for i, s in enumerate(up)]
        res = lambda: dict(down_block_add_samples=[r.clone() for r in down], mid_block_add_sample=mid.clone(),
                           up_block_add_samples=[r.clone() for r in up])
        unet, _ = build_tiny()
        unet._load_ip_adapter_weights([tiny_ip_adapter(i) for i in range(len(images))], low_cpu_mem_usage=False)
        for p in unet.attn_processors.values():
            if isinstance(p, IPAdapterAttnProcessor2_0):
                p.scale = list(IP_UNET_SCALES[case])

        def run(masks):
            with torch.no_grad():
                return unet(x_u, t, encoder_hidden_states=ehs, added_cond_kwargs={"image_embeds": embeds}, return_dict=False,
                            **({} if masks is None else dict(cross_attention_kwargs={"ip_adapter_masks": masks})), **res())[0].numpy()
        masks = unet_masks(case)
        eps = run(None)
        assert np.array_equal(eps, base[f"{case}_eps"]), "without masks: the eps of unet_tiny_ip.npz, bit for bit"
        got = {"eps": eps, "eps_masked": run(masks)}
        if any(n > 1 for n in images):
            got["eps_swapped"] = run(swap_images(masks))
        tags = list(got)
        gaps = {a + "/" + b: rel(got[a], got[b]) / 1e-2 for i, a in enumerate(tags) for b in tags[i + 1:]}
        print(f"ip-adapter masks UNet {case}: eps std {got['eps_masked'].std():.4f}, variants apart by {gaps} bars")
        assert min(gaps.values()) >= 10.0, (case, gaps)
        out.update({f"{case}_{k}": v for k, v in got.items() if k != "eps"})
    np.savez_compressed(os.path.join(OUT, "unet_tiny_ip_masks.npz"), **out)
    print("unet_tiny_ip_masks.npz: %.1f KB" % (os.path.getsize(os.path.join(OUT, "unet_tiny_ip_masks.npz")) / 1024))


def golden_pipeline_call_ip_masks():
    """tests/golden/pipeline_call_ip_masks.npz: the call of golden_pipeline_call_ip (same seeds, adapter, scale IP_CALL_SCALE and
    embeddings) with cross_attention_kwargs={"ip_adapter_masks": [...]} (pipe:1084).  The stored uint8 mask images (`mask_A`, `mask_B`,
    tests/ip_masks_common.py call_mask_images; 64 x 128, the aspect ratio of the canvas the UNet runs on) go through the reference's
    IPAdapterMaskProcessor.preprocess(mask, 64, 128); the preprocessed masks are stored too (`pre_A`, `pre_B`, fp32 [1][1][64][128]),
    with the preprocessed masks of the same images at half the size (`pre_A_32x64`: lanczos, then binarised).  Latents for mask A, for
    mask B and - asserted equal to pipeline_call_ip.npz's - without masks; at least 10 GPU bars (1e-2 of the latents' scale) apart."""
    import warnings
    from PIL import Image
    from diffusers.image_processor import IPAdapterMaskProcessor
    from diffusers.loaders.ip_adapter import IPAdapterMixin
    from diffusers.pipelines.stable_diffusion.pipeline_stable_diffusion import StableDiffusionPipeline
    from tests.common import FakeTokenizer, pipeline_cases
    from tests.ip_adapter_common import IP_CALL_SCALE, ip_call_embeds, tiny_ip_adapter
    from tests.ip_masks_common import call_mask_images
    base = np.load(os.path.join(OUT, "pipeline_call.npz"))
    zi = np.load(os.path.join(OUT, "pipeline_call_ip.npz"))
    kw = dict(pipeline_cases()["ddim_neg2"])
    for k in ("scheduler", "seed", "rng_seed"):
        kw.pop(k)
    kw["num_inference_steps"] = int(zi["num_inference_steps"])
    seed, rng_seed = int(zi["seed"]), int(zi["rng_seed"])
    embeds = ip_call_embeds()
    unet, blob, vae, te, proc, dino = _tiny_pipeline_components()
    unet._load_ip_adapter_weights([tiny_ip_adapter(0)], low_cpu_mem_usage=False)
    sch = DDIMScheduler(**SD_SCHED, clip_sample=False, set_alpha_to_one=False)
    pipe = StableDiffusionBlobNetPipeline(vae=vae, unet=unet, tokenizer=FakeTokenizer(), text_encoder=te, blobnet=blob, scheduler=sch,
                                          safety_checker=None, dinov2_processor=proc, dinov2=dino, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    pipe.prepare_ip_adapter_image_embeds = types.MethodType(StableDiffusionPipeline.prepare_ip_adapter_image_embeds, pipe)
    IPAdapterMixin.set_ip_adapter_scale(pipe, IP_CALL_SCALE)
    mp = IPAdapterMaskProcessor()
    images = call_mask_images()
    out = {}
    for tag, im in images.items():
        out[f"mask_{tag}"] = im.astype(np.uint8)
        pre = mp.preprocess(Image.fromarray(out[f"mask_{tag}"]), height=64, width=128)
        out[f"pre_{tag}"] = pre.reshape(1, pre.shape[0], pre.shape[2], pre.shape[3]).numpy()
        half = mp.preprocess(Image.fromarray(out[f"mask_{tag}"]), height=32, width=64)
        out[f"pre_{tag}_32x64"] = half.reshape(1, half.shape[0], half.shape[2], half.shape[3]).numpy()
        assert set(np.unique(out[f"pre_{tag}"])) == {0.0, 1.0} and out[f"pre_{tag}"].shape == (1, 1, 64, 128)

    def call(masks):
        torch.manual_seed(rng_seed)
        with warnings.catch_warnings():
            warnings.simplefilter("error", UserWarning)                   # (no level pads: the masks have the canvas' aspect ratio)
            return pipe(fg_image=Image.fromarray(base["fg"]), bg_image=Image.fromarray(base["bg"]), gs_score=torch.from_numpy(base["gs_score"]),
                        height=64, width=64, generator=torch.Generator().manual_seed(seed), output_type="latent",
                        ip_adapter_image_embeds=[embeds], **({} if masks is None else dict(cross_attention_kwargs={"ip_adapter_masks": masks})),
                        **kw).images.numpy()
    out["latents_none"] = call(None)
    assert np.array_equal(out["latents_none"], zi["latents"]), "without masks: the latents of pipeline_call_ip.npz, bit for bit"
    for tag in images:
        out[f"latents_{tag}"] = call([torch.from_numpy(out[f"pre_{tag}"])])
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    gaps = (rel(out["latents_A"], out["latents_B"]), rel(out["latents_A"], out["latents_none"]), rel(out["latents_B"], out["latents_none"]))
    print("pipeline __call__ ip-adapter masks: latents std %.4f; A vs B %.3f, A vs none %.3f, B vs none %.3f (max-abs / scale)" %
          ((out["latents_A"].std(),) + gaps))
    assert min(gaps) >= 10 * 1e-2, gaps
    np.savez_compressed(os.path.join(OUT, "pipeline_call_ip_masks.npz"), **out)
    print("pipeline_call_ip_masks.npz: %.1f KB" % (os.path.getsize(os.path.join(OUT, "pipeline_call_ip_masks.npz")) / 1024))


TINY_VAE_CASES = {"a": (2, 5, 7), "b": (1, 1, 1), "c": (3, 9, 3)}      # tag -> (batch, latent h, w); seeds 331 ... in this order


def golden_tiny_vae():
    """tests/golden/autoencoder_tiny.npz: the reference's AutoencoderTiny (default architecture) with synth weights, seed 33, on z = 2 N(0, 1):
    `<tag>_z`, `<tag>_sample` = decode(z).sample, `<tag>_preview` = the bytes round(clamp(sample / 2 + 0.5, 0, 1) * 255) as [B][H][W][3]; `schema`
    = the (name, shape) list of the reference's decoder state dict; `meta` (JSON) = the per-layer output stds of case a, the share of
    saturated preview bytes, and the error of an fp16-storage emulation of the reference (weights, inputs and every Conv2d / ReLU output
    rounded to fp16, arithmetic in fp32 on the CPU) per case.  synth's N(0, 1 / fan_in) weights, NOT the framework's default initialisation:
    with that the image's std falls to 0.04 and an error in a layer no longer reaches the output."""
    from diffusers import AutoencoderTiny
    vae = AutoencoderTiny().eval()
    sh = synth.tiny_vae_param_shapes()
    dec = {"decoder." + k: tuple(v.shape) for k, v in vae.decoder.state_dict().items()}
    assert list(dec) == list(sh) and all(dec[k] == tuple(sh[k]) for k in dec), "AutoencoderTiny decoder schema mismatch"
    sd = synth.synth_state_dict(sh, 33)
    vae.decoder.load_state_dict({k[len("decoder."):]: v for k, v in sd.items()}, strict=True)
    out = {"schema": np.array(json.dumps([[k, list(v)] for k, v in dec.items()]))}
    mods = [m for m in vae.decoder.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.ReLU))]
    stds, hooks = [], [m.register_forward_hook(lambda _m, _i, o: stds.append(float(o.std()))) for m in mods if isinstance(m, torch.nn.Conv2d)]
    meta = {"cases": {}, "seed": 33}
    for n, (tag, (B, h, w)) in enumerate(TINY_VAE_CASES.items()):
        z = 2.0 * g(331 + n, B, 4, h, w)
        del stds[:]
        sample = vae.decode(z).sample
        if tag == "a":
            meta["layer_output_std"] = list(stds)
        by = ((sample / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        out[f"{tag}_z"], out[f"{tag}_sample"], out[f"{tag}_preview"] = z.numpy(), sample.numpy(), by.numpy()
        meta["cases"][tag] = dict(shape=[B, h, w], sample_std=float(sample.std()), sample_max_abs=float(sample.abs().max()),
                                  saturated_bytes=float(((by == 0) | (by == 255)).float().mean()))
    for hk in hooks:
        hk.remove()
    # fp16-storage emulation
    keep = {k: v.clone() for k, v in vae.decoder.state_dict().items()}
    vae.decoder.load_state_dict({k: (v.half().float() if k.endswith("weight") else v) for k, v in keep.items()}, strict=True)
    hooks = [m.register_forward_hook(lambda _m, _i, o: o.half().float()) for m in mods]
    hooks.append(vae.decoder.layers.register_forward_pre_hook(lambda _m, i: (i[0].half().float(),)))
    for tag in TINY_VAE_CASES:
        emu = vae.decode(torch.from_numpy(out[f"{tag}_z"])).sample.numpy()
        ref = out[f"{tag}_sample"]
        meta["cases"][tag]["fp16_storage_emulation_max_abs_over_scale"] = float(np.abs(emu - ref).max() / np.abs(ref).max())
    for hk in hooks:
        hk.remove()
    vae.decoder.load_state_dict(keep, strict=True)
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(OUT, "autoencoder_tiny.npz")
    np.savez_compressed(path, **out)
    lo, hi = min(meta["layer_output_std"]), max(meta["layer_output_std"])
    print("autoencoder_tiny.npz: %.1f KB; layer stds %.3f .. %.3f; %s" % (os.path.getsize(path) / 1024, lo, hi, json.dumps(meta["cases"])))
    assert 0.2 < lo and hi < 1.6, "a decoder layer's output has left the O(1) range: an error there would not reach the image"


# ------------------------------------------------------------------------------------------------ perturbed-attention guidance (PAG)
def _pag_shim(unet, layers, pag_scale=3.0, pag_adaptive_scale=0.0):
    """A PAGMixin object around `unet`, as the reference's PAG pipelines are one: set_pag_applied_layers has run."""
    from diffusers.pipelines.pag.pag_utils import PAGMixin
    shim = type("PagShim", (PAGMixin,), {})()
    shim.unet, shim._pag_scale, shim._pag_adaptive_scale = unet, pag_scale, pag_adaptive_scale
    shim.set_pag_applied_layers(layers)
    return shim


def _pag_gain(unet):
    """The one changed weight of the PAG fixtures (tests/pag_common.py pag_tiny_unet_weights) on a reference UNet; returns it."""
    from tests.pag_common import PAG_MID_VALUE_GAIN, PAG_MID_VALUE_KEY
    sd = unet.state_dict()
    sd[PAG_MID_VALUE_KEY] = sd[PAG_MID_VALUE_KEY] * PAG_MID_VALUE_GAIN
    unet.load_state_dict(sd, strict=True)
    return unet


def _pag_names(unet):
    from diffusers.models.attention_processor import PAGCFGIdentitySelfAttnProcessor2_0, PAGIdentitySelfAttnProcessor2_0
    return [n for n, m in unet.named_modules() if isinstance(getattr(m, "processor", None), (PAGCFGIdentitySelfAttnProcessor2_0, PAGIdentitySelfAttnProcessor2_0))]


def golden_blocks_pag():
    """tests/golden/blocks_pag.npz: one Transformer2DModel at 320, 640 and 1280 channels with PAGCFGIdentitySelfAttnProcessor2_0 on attn1
    (batch [uncond | cond | perturbed]) and one case with PAGIdentitySelfAttnProcessor2_0 ([cond | perturbed]) - tests/pag_common.py
    PAG_BLOCK_CASES.  The cond and perturbed chunks get identical inputs; their outputs must lie at least 10 times the GPU bar of
    tests/test_blocks_gpu.py (1e-2 of the output's max-abs) apart, or the fixture could not see a missing perturbation.  Outputs only
    (fp32, every `sub`-th pixel); weights and inputs come from seeds on both sides."""
    from diffusers.models.attention_processor import PAGCFGIdentitySelfAttnProcessor2_0, PAGIdentitySelfAttnProcessor2_0
    from diffusers.models.transformers.transformer_2d import Transformer2DModel
    from tests.pag_common import PAG_BLOCK_CASES, pag_block_inputs, pag_block_weights
    out = {}
    for name, p in PAG_BLOCK_CASES.items():
        x, ctx = pag_block_inputs(name)
        m = Transformer2DModel(num_attention_heads=p["heads"], attention_head_dim=p["C"] // p["heads"], in_channels=p["C"], num_layers=1,
                               cross_attention_dim=p["ctx"], norm_num_groups=32).eval()
        m.load_state_dict(pag_block_weights(name), strict=True)
        m.transformer_blocks[0].attn1.set_processor(PAGCFGIdentitySelfAttnProcessor2_0() if p["chunks"] == 3 else PAGIdentitySelfAttnProcessor2_0())
        with torch.no_grad():
            y = m(x, encoder_hidden_states=ctx, return_dict=False)[0].numpy().astype(np.float32)
        n = p["B"] // p["chunks"]
        gap = float(np.abs(y[-n:] - y[-2 * n:-n]).max() / (1e-2 * np.abs(y).max()))
        print(f"block {name}: out std {y.std():.4f}, perturbed vs cond chunk {gap:.1f} bars apart")
        assert gap >= 10.0, (name, gap)
        out[name] = y[:, :, ::p["sub"], ::p["sub"]]
    path = os.path.join(OUT, "blocks_pag.npz")
    np.savez_compressed(path, **out)
    print("blocks_pag.npz: %.1f KB" % (os.path.getsize(path) / 1024))


def golden_unet_pag():
    """tests/golden/unet_tiny_pag.npz: the tiny UNet of build_tiny() at batch 3 = [uncond | cond | perturbed] (tests/pag_common.py
    pag_unet_inputs, residual stand-ins pag_residual) with the processors PAGMixin._set_pag_attn_processor sets for PAG_UNET_LAYERS:
    `eps_<case>` and `eps_off` (no PAG processor), at least 10 times the GPU bar (1e-2 of eps' scale, tests/test_freeu_gpu.py) apart.
    The UNet carries the one changed weight of pag_tiny_unet_weights (see there).
    Also the module names the reference matches for every id of PAG_MATCH_IDS (`match_<i>`: a JSON list, empty where it raises
    ValueError) and `_get_pag_scale` over PAG_SCALE_TIMESTEPS for PAG_SCALE_CASES (`scale_<case>`)."""
    from tests.pag_common import (PAG_MATCH_IDS, PAG_SCALE_CASES, PAG_SCALE_TIMESTEPS, PAG_UNET_GEOMETRY, PAG_UNET_LAYERS, pag_residual,
                                  pag_unet_inputs)
    _, H, W = PAG_UNET_GEOMETRY
    x, ehs, seed = pag_unet_inputs()
    t = torch.tensor(981)
    down, mid, up = _freeu_residual_shapes(H, W)
    down, mid, up = [pag_residual(seed + i, s) for i, s in enumerate(down)], pag_residual(seed + 100, mid), [pag_residual(seed + 200 + i, s) for i, s in enumerate(up)]
    res = lambda: dict(down_block_add_samples=[r.clone() for r in down], mid_block_add_sample=mid.clone(), up_block_add_samples=[r.clone() for r in up])
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    run = lambda u: u(x, t, encoder_hidden_states=ehs, return_dict=False, **res())[0].numpy()
    out = {"timestep": np.array(981), "eps_off": run(_pag_gain(build_tiny()[0]))}
    assert np.array_equal(out["eps_off"][1], out["eps_off"][2]), "cond and perturbed images are identical without PAG"
    for case, layers in PAG_UNET_LAYERS.items():
        unet = _pag_gain(build_tiny()[0])
        shim = _pag_shim(unet, layers)
        shim._set_pag_attn_processor(shim.pag_applied_layers, True)
        out[f"eps_{case}"] = eps = run(unet)
        out[f"names_{case}"] = np.array(json.dumps(_pag_names(unet)))
        gap = rel(eps, out["eps_off"]) / 1e-2
        print(f"PAG UNet {case}: {len(_pag_names(unet))} layers, eps std {eps.std():.4f}, on vs off {gap:.1f} bars; uncond / cond rows equal off: "
              f"{np.array_equal(eps[:2], out['eps_off'][:2])}")
        assert gap >= 10.0 and np.array_equal(eps[:2], out["eps_off"][:2]), (case, gap)
    for i, layer_id in enumerate(PAG_MATCH_IDS):
        unet, _ = build_tiny()
        shim = _pag_shim(unet, layer_id)
        try:
            shim._set_pag_attn_processor(shim.pag_applied_layers, True)
            names = _pag_names(unet)
            assert names
        except ValueError:
            names = []
        out[f"match_{i}"] = np.array(json.dumps(names))
        print(f"PAG layer id {layer_id!r}: {len(names)} modules")
    out["match_ids"] = np.array(json.dumps(list(PAG_MATCH_IDS)))
    for case, (s, a) in PAG_SCALE_CASES.items():
        shim = _pag_shim(build_tiny()[0], "mid", s, a)
        out[f"scale_{case}"] = np.array([float(shim._get_pag_scale(torch.tensor(ts))) for ts in PAG_SCALE_TIMESTEPS], dtype=np.float64)
    assert out["scale_clamped"].min() == 0.0 and out["scale_clamped"].max() > 0.0
    path = os.path.join(OUT, "unet_tiny_pag.npz")
    np.savez_compressed(path, **out)
    print("unet_tiny_pag.npz: %.1f KB" % (os.path.getsize(path) / 1024))


def _pag_wrap_unet(unet, shim, guidance_scale, do_cfg):
    """Make the reference pipeline's own loop compute PAG: `unet.forward` of this instance takes the call's batch - [uncond | cond], or
    [cond] without classifier-free guidance - runs the real forward with the PAG processors on [uncond | cond | cond] ([cond | cond]),
    every per-image argument and BlobNet add-sample duplicated the way _prepare_perturbed_attention_guidance duplicates `cond`, and hands
    back [e_u | e_c + (s / g) (e_c - e_p)], so that the pipeline's e_u + g (e'_c - e_u) is e_u + g (e_c - e_u) + s (e_c - e_p); without
    CFG it hands back e_c + s (e_c - e_p).  s = _get_pag_scale(t)."""
    shim._set_pag_attn_processor(shim.pag_applied_layers, do_cfg)
    inner = type(unet).forward

    def forward(self, sample, timestep, encoder_hidden_states, timestep_cond=None, cross_attention_kwargs=None, down_block_add_samples=None,
                mid_block_add_sample=None, up_block_add_samples=None, added_cond_kwargs=None, return_dict=False, **kw):
        assert not kw and not return_dict
        n = sample.shape[0] // (2 if do_cfg else 1)
        dup = lambda v: None if v is None else torch.cat([v, v[-n:]], 0)
        added = None if added_cond_kwargs is None else {k: [dup(e) for e in v] if isinstance(v, list) else dup(v) for k, v in added_cond_kwargs.items()}
        eps = inner(self, dup(sample), timestep, dup(encoder_hidden_states), timestep_cond=dup(timestep_cond),
                    cross_attention_kwargs=cross_attention_kwargs, down_block_add_samples=[dup(r) for r in down_block_add_samples],
                    mid_block_add_sample=dup(mid_block_add_sample), up_block_add_samples=[dup(r) for r in up_block_add_samples],
                    added_cond_kwargs=added, return_dict=False)[0]
        s = float(shim._get_pag_scale(timestep))
        if do_cfg:
            eu, ec, ep = eps.chunk(3)
            return (torch.cat([eu, ec + (s / guidance_scale) * (ec - ep)], 0),)
        ec, ep = eps.chunk(2)
        return (ec + s * (ec - ep),)
    unet.forward = types.MethodType(forward, unet)


def golden_pipeline_call_pag():
    """tests/golden/pipeline_call_pag.npz: the reference's own `__call__` (pipe:743-1166) on the tiny pipeline of pipeline_call_ip.npz
    (case `ddim_neg2` of pipeline_call.npz, 3 steps, seeds of its own; the UNet with the one changed weight of pag_tiny_unet_weights) with its UNet wrapped by _pag_wrap_unet - the loop is the
    reference's, only the UNet call computes the PAG batch.  Cases (tests/pag_common.py PAG_CALL_CASES): DDIM with PAG on
    "mid", with an adaptive scale, with half the scale, PAG off, guidance-free (guidance_scale 1.0) with and without PAG, and
    EulerDiscreteScheduler (a table that scales the model input) with and without PAG.  The pairs of PAG_CALL_PAIRS lie at least 10 times
    the GPU bar (1e-2 of the latents' scale) apart."""
    from PIL import Image
    from diffusers import EulerDiscreteScheduler
    from tests.common import FakeTokenizer, pipeline_cases
    from tests.pag_common import PAG_CALL_CASES, PAG_CALL_LAYERS, PAG_CALL_PAIRS, PAG_CALL_SEEDS
    base = np.load(os.path.join(OUT, "pipeline_call.npz"))
    kw0 = dict(pipeline_cases()["ddim_neg2"])
    for k in ("scheduler", "seed", "rng_seed"):
        kw0.pop(k)
    kw0["num_inference_steps"] = 3
    seed, rng_seed = PAG_CALL_SEEDS["seed"], PAG_CALL_SEEDS["rng_seed"]
    out = {"seed": np.array(seed), "rng_seed": np.array(rng_seed), "num_inference_steps": np.array(3)}
    for case, extra in PAG_CALL_CASES.items():
        kw = dict(kw0)
        kw["guidance_scale"] = extra.get("guidance_scale", kw0["guidance_scale"])
        unet, blob, vae, te, proc, dino = _tiny_pipeline_components()
        _pag_gain(unet)
        sch = DDIMScheduler(**SD_SCHED, clip_sample=False, set_alpha_to_one=False)
        if case.startswith("euler"):
            sch = EulerDiscreteScheduler.from_config(sch.config)
        pipe = StableDiffusionBlobNetPipeline(vae=vae, unet=unet, tokenizer=FakeTokenizer(), text_encoder=te, blobnet=blob, scheduler=sch,
                                              safety_checker=None, dinov2_processor=proc, dinov2=dino, requires_safety_checker=False)
        pipe.set_progress_bar_config(disable=True)
        if extra.get("pag_scale", 0.0) > 0:
            shim = _pag_shim(unet, PAG_CALL_LAYERS, extra["pag_scale"], extra.get("pag_adaptive_scale", 0.0))
            _pag_wrap_unet(unet, shim, kw["guidance_scale"], kw["guidance_scale"] > 1.0)
        torch.manual_seed(rng_seed)
        out[f"{case}_latents"] = pipe(fg_image=Image.fromarray(base["fg"]), bg_image=Image.fromarray(base["bg"]),
                                      gs_score=torch.from_numpy(base["gs_score"]), height=64, width=64,
                                      generator=torch.Generator().manual_seed(seed), output_type="latent", **kw).images.numpy()
        out[f"{case}_timesteps"] = pipe.scheduler.timesteps.numpy()
        print(f"pipeline __call__ PAG {case}: latents std {out[f'{case}_latents'].std():.4f}")
    rel = lambda a, b: float(np.abs(out[f"{a}_latents"] - out[f"{b}_latents"]).max() / np.abs(out[f"{b}_latents"]).max())
    gaps = {f"{a}/{b}": rel(a, b) / 1e-2 for a, b in PAG_CALL_PAIRS}
    print("pipeline __call__ PAG: variants apart by (bars)", {k: round(v, 1) for k, v in gaps.items()})
    assert min(gaps.values()) >= 10.0, gaps
    path = os.path.join(OUT, "pipeline_call_pag.npz")
    np.savez_compressed(path, **out)
    print("pipeline_call_pag.npz: %.1f KB" % (os.path.getsize(path) / 1024))


# ------------------------------------------------------------------------------------------------ masked edits (latent blend)
_BLEND_NOISE_MODULES = {"ddim": "diffusers.schedulers.scheduling_ddim", "sde": "diffusers.schedulers.scheduling_dpmsolver_multistep",
                        "eulera": EULER_A_MODULE, "lcm": LCM_MODULE}


def golden_pipeline_call_blend():
    """tests/golden/pipeline_call_blend.npz: the reference's own `__call__` (pipe:743-1166) on the tiny pipeline of pipeline_call.npz (case
    `ddim_neg2`, 64 x 64, 3 steps - 5 for DPM-Solver++ 3M, whose table has no third-order row below that - `latents=` given) as a masked edit and as a plain one, per case of tests/blend_common.py BLEND_CASES.  The
    blend is the inpainting pipeline's (pipeline_stable_diffusion_inpaint.py:1272-1285) with the reference scheduler's own add_noise,
    applied to what `scheduler.step` returns (pipe:1102).  That is where a callback_on_step_end would apply it - nothing stands between the
    two - but the reference's callback branch reads names its `__call__` never binds (pipe:1115-1116) and cannot be entered.  Stored per
    case: the final latents with and without the blend, the timesteps, and of the blended run the guided eps, the sample entering and the
    blended latents leaving every step, the noise a stochastic step drew and the add_noise coefficients (a, s) of every step.
    A second file, blend_mask.npz: the reference's mask_processor + prepare_mask_latents reduction of an odd uint8 mask holding bytes 127
    and 128."""
    import diffusers as ref_mod
    from PIL import Image
    from tests.common import FakeTokenizer, pipeline_cases
    from tests import blend_common as bc
    base = np.load(os.path.join(OUT, "pipeline_call.npz"))
    kw0 = dict(pipeline_cases()["ddim_neg2"])
    for k in ("scheduler", "seed", "rng_seed"):
        kw0.pop(k)
    kw0["num_inference_steps"] = bc.BLEND_STEPS
    seed, rng_seed = bc.BLEND_SEEDS["seed"], bc.BLEND_SEEDS["rng_seed"]
    out = {"seed": np.array(seed), "rng_seed": np.array(rng_seed), "num_inference_steps": np.array(bc.BLEND_STEPS), "mask": bc.BLEND_MASK}
    assert 64 / 3 <= bc.BLEND_MASK.sum() <= 128 / 3 and not np.array_equal(bc.BLEND_MASK, bc.BLEND_MASK.T)
    unet, blob, vae, te, proc, dino = _tiny_pipeline_components()
    for case, extra in bc.BLEND_CASES.items():
        kw = dict(kw0, **{k: v for k, v in extra.items() if k != "scheduler"})
        batch = len(kw["prompt"]) * kw.get("num_images_per_prompt", 1)
        lat, image, mask = bc.blend_inputs(batch)
        for blended in (True, False):
            sch = bc.make_scheduler(ref_mod, extra["scheduler"], SD_SCHED)
            pipe = StableDiffusionBlobNetPipeline(vae=vae, unet=unet, tokenizer=FakeTokenizer(), text_encoder=te, blobnet=blob,
                                                  scheduler=sch, safety_checker=None, dinov2_processor=proc, dinov2=dino,
                                                  requires_safety_checker=False)
            pipe.set_progress_bar_config(disable=True)
            tap = dict(eps=[], x=[], out=[], coef=[])
            step = sch.step

            def blended_step(model_output, t, sample, *a, _step=step, _sch=sch, **k_):
                i = len(tap["eps"])
                prev = _step(model_output, t, sample, *a, **k_)[0]
                ts = _sch.timesteps
                proper, row = image, (1.0, 0.0)
                if i < len(ts) - 1:                                        # inpaint:1272-1285
                    t_next = ts[i + 1: i + 2]
                    proper = _sch.add_noise(image, lat, t_next)
                    one, zero = torch.ones(1, 1, 1, 1), torch.zeros(1, 1, 1, 1)
                    row = (float(_sch.add_noise(one, zero, t_next)), float(_sch.add_noise(zero, one, t_next)))
                prev = (1 - mask) * proper + mask * prev
                for key, v in (("eps", model_output), ("x", sample), ("out", prev)):
                    tap[key].append(v.detach().clone())
                tap["coef"].append(row)
                return (prev,)
            blended_step.__wrapped__ = step                                # (prepare_extra_step_kwargs inspects the signature for eta / generator)
            if blended:
                sch.step = blended_step
            torch.manual_seed(rng_seed)
            kind = extra["scheduler"]
            module = _BLEND_NOISE_MODULES.get(kind) if (kind != "ddim" or extra.get("eta")) else None
            noise = _TapNoise(module) if module else None
            if noise:
                noise.__enter__()
            try:
                r = pipe(fg_image=Image.fromarray(base["fg"]), bg_image=Image.fromarray(base["bg"]), gs_score=torch.from_numpy(base["gs_score"]),
                         height=64, width=64, latents=lat.clone(), generator=torch.Generator().manual_seed(seed), output_type="latent", **kw)
            finally:
                if noise:
                    noise.__exit__()
            tag = f"{case}_blend" if blended else f"{case}_plain"
            out[f"{tag}_latents"] = r.images.numpy()
            if blended:
                assert len(tap["eps"]) == kw["num_inference_steps"]
                out[f"{case}_timesteps"] = sch.timesteps.numpy()
                out[f"{case}_step_eps"], out[f"{case}_step_in"], out[f"{case}_step_out"] = (torch.stack(tap[k_]).numpy() for k_ in ("eps", "x", "out"))
                out[f"{case}_add_noise"] = np.array(tap["coef"], dtype=np.float32)
                if noise:
                    out[f"{case}_step_noise"] = torch.stack(noise.drawn).numpy()
                keep = (mask == 0).expand_as(image).numpy()
                assert np.array_equal(out[f"{tag}_latents"][keep], image.numpy()[keep]), case        # exactly the image outside the mask
        a, b = out[f"{case}_blend_latents"], out[f"{case}_plain_latents"]
        gap = float(np.abs(a - b).max() / np.abs(b).max()) / 1e-2
        print(f"pipeline __call__ blend {case}: latents std {a.std():.4f}, blend vs plain {gap:.1f} bars")
        assert gap >= 10.0, (case, gap)
    # the mask path: mask_processor (no normalise, binarise, greyscale) + prepare_mask_latents' default-mode F.interpolate
    from diffusers.image_processor import VaeImageProcessor
    rng = np.random.Generator(np.random.PCG64(41))
    m8 = rng.integers(0, 256, (48, 72)).astype(np.uint8)
    m8[::8, ::8][0, :4] = (127, 128, 0, 255)
    m8[8, 8], m8[16, 24] = 127, 128
    proc_m = VaeImageProcessor(vae_scale_factor=8, do_normalize=False, do_binarize=True, do_convert_grayscale=True)
    full = proc_m.preprocess(Image.fromarray(m8), height=48, width=72)
    assert (m8[::8, ::8] == 127).any() and (m8[::8, ::8] == 128).any()
    np.savez_compressed(os.path.join(OUT, "blend_mask.npz"), mask_u8=m8, mask_processed=full.numpy(),
                        mask_latent=torch.nn.functional.interpolate(full, size=(6, 9)).numpy())
    path = os.path.join(OUT, "pipeline_call_blend.npz")
    np.savez_compressed(path, **out)
    print("pipeline_call_blend.npz: %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    if len(sys.argv) > 1:
        if sys.argv[1] == "golden_fullsize_loop":             # python tools/make_golden.py golden_fullsize_loop [unipc:1.0 ...]
            golden_fullsize_loop(sys.argv[2:] or None)
            sys.exit(0)
        if sys.argv[1] == "golden_config_loops":              # python tools/make_golden.py golden_config_loops [c5 c3_r0 c3_r1]
            golden_config_loops(sys.argv[2:] or None)
            sys.exit(0)
        for fn in sys.argv[1:]:
            globals()[fn]()
        sys.exit(0)
    check_full_schema()
    golden_pipeline_call()
    golden_lora_keys()
    golden_lora_kohya()
    golden_lora_merge()
    golden_blob_edit()
    golden_blob_edit_cv()
    golden_clip_text()
    golden_vae()
    golden_splat()
    golden_blob_viz()
    golden_schedulers()
    golden_dinov2()
    golden_sam()
    golden_nets()
    golden_loop()
    golden_blocks()
    golden_schedulers_eta()
    golden_loop_eta()
    golden_pipeline_call_eta()
    golden_schedulers_dpm()
    golden_loop_dpm()
    golden_pipeline_call_dpm()
    golden_schedulers_euler()
    golden_loop_euler()
    golden_pipeline_call_euler()
    golden_schedulers_lcm()
    golden_loop_lcm()
    golden_unet_timecond()
    golden_pipeline_call_lcm()
    golden_freeu()
    golden_pipeline_call_freeu()
    golden_blocks_ip()
    golden_ip_adapter()
    golden_pipeline_call_ip()
    golden_ip_plus()
    golden_clip_vision()
    golden_clip_processor()
    golden_pipeline_call_ip_image()
    golden_overlay()
    golden_ip_mask_downsample()
    golden_blocks_ip_masks()
    golden_unet_ip_masks()
    golden_pipeline_call_ip_masks()
    golden_tiny_vae()
    golden_blocks_pag()
    golden_unet_pag()
    golden_pipeline_call_pag()
    golden_pipeline_call_blend()
    print("golden fixtures written to", OUT)
    for f in sorted(os.listdir(OUT)):
        print("  %-24s %8.1f KB" % (f, os.path.getsize(os.path.join(OUT, f)) / 1024))
