"""LCMScheduler and single-pass plans, host side: the timestep schedules, `.config`, step trajectories and noise draws of the REFERENCE's
LCMScheduler (tests/golden/schedulers_lcm.npz, lcm_config.json, loop_tiny_lcm.npz, pipeline_call_lcm.npz), every refusal, and what
compiled plans launch: a guidance-free LCM edit runs the UNet at batch B and ends its steps in bc_scheduler_step_single (a version-7
file), while every configuration that existed before compiles to the listing it always had (plan_listings_before_lcm.json: listings
written by the commit before this scheduler)."""
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests.common import TINY, build_plan_dump, g, plan_named as _named, plan_stored as _stored, tiny_weights

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000, steps_offset=1)
OP_STEP, OP_STEP_NOISE, OP_STEP_SINGLE, OP_TEMB_TABLE = 11, 30, 34, 10


def _gold(name):
    return np.load(os.path.join(GOLD, name))


def _cases(z):
    return sorted(k[:-3] for k in z.files if k.endswith("_kw"))


def _lcm(**kw):
    from blobctrl_amd.schedulers import LCMScheduler
    return LCMScheduler(**dict(SD, set_alpha_to_one=False, **kw))


# ------------------------------------------------------------------------------------------------------------ scheduler
def test_timesteps_equal_the_reference():
    z = _gold("schedulers_lcm.npz")
    assert len(_cases(z)) == 11
    for name in _cases(z):
        kw = json.loads(str(z[f"{name}_kw"]))
        s = _lcm(**kw["options"])
        s.set_timesteps(**kw["set_timesteps"])
        assert s.timesteps.dtype == torch.int64 and np.array_equal(s.timesteps.numpy(), z[f"{name}_timesteps"]), name
        x = torch.from_numpy(z[f"{name}_traj"][0])
        assert s.init_noise_sigma == 1 and s.order == 1 and s.scale_model_input(x, s.timesteps[0]) is x
    s = _lcm()
    s.set_timesteps(4)
    assert s.timesteps.tolist() == [999, 759, 499, 259]


def test_config_equals_the_reference():
    from blobctrl_amd.schedulers import (DDIMScheduler, DPMSolverMultistepScheduler, LCMScheduler, PNDMScheduler, UniPCMultistepScheduler,
                                         scheduler_from_config_dir)
    ref = json.load(open(os.path.join(GOLD, "lcm_config.json")))
    s = LCMScheduler.from_config(ref["source"])
    cfg = dict(s.config)
    cfg["_use_default_values"] = sorted(cfg["_use_default_values"])
    assert cfg == ref["lcm"]
    assert (cfg["original_inference_steps"], cfg["timestep_scaling"], cfg["timestep_spacing"], cfg["steps_offset"], cfg["set_alpha_to_one"]) == \
        (50, 10.0, "leading", 1, False)
    p = PNDMScheduler(**{k: v for k, v in ref["source"].items() if not k.startswith("_") and k != "trained_betas"})
    for src in (p, DDIMScheduler.from_config(p.config), DPMSolverMultistepScheduler.from_config(p.config)):
        s2 = LCMScheduler.from_config(src.config)
        for k in set(LCMScheduler._defaults) | set(SD) | {"prediction_type"}:
            assert s2.config[k] == ref["lcm"][k], (type(src).__name__, k)
        assert s2.kind == "lcm" and s2.table_params()[:3] == (1000, 0.00085, 0.012) and s2.table_params()[3] == (("original_inference_steps", 50), ("set_alpha_to_one", False),
                                                               ("timestep_scaling", 10.0))
    # (a UniPC config has no set_alpha_to_one to hand on: the class default holds, as for any key the source does not have)
    assert LCMScheduler.from_config(UniPCMultistepScheduler.from_config(p.config).config).config.steps_offset == 1
    d = LCMScheduler()                                            # the reference's own defaults (scheduling_lcm.py:196-215)
    assert (d.config.set_alpha_to_one, d.config.steps_offset, d.config.original_inference_steps, d.config.timestep_scaling,
            d.config.clip_sample, d.config.thresholding) == (True, 0, 50, 10.0, False, False)
    k = LCMScheduler.from_config(p.config, original_inference_steps=30)
    assert k.config.original_inference_steps == 30 and "original_inference_steps" not in k.config._use_default_values
    import copy
    copy.deepcopy(k)


def test_scheduler_from_config_dir_knows_the_class(tmp_path):
    from blobctrl_amd.schedulers import LCMScheduler, OPTION_KINDS, LCMTable, scheduler_from_config_dir, table_class
    json.dump({"_class_name": "LCMScheduler", "beta_start": 0.00085, "beta_end": 0.012, "beta_schedule": "scaled_linear",
               "num_train_timesteps": 1000, "original_inference_steps": 40, "timestep_scaling": 10.0},
              open(tmp_path / "scheduler_config.json", "w"))
    s = scheduler_from_config_dir(str(tmp_path))
    assert isinstance(s, LCMScheduler) and s.config.original_inference_steps == 40
    assert table_class("lcm") is LCMTable and "lcm" in OPTION_KINDS and LCMTable.sde


def test_host_step_trajectories_match_the_reference():
    """rtol / atol 2e-5 (the bar tests/test_kernels_gpu.py holds step trajectories to), with the reference's noise given."""
    z = _gold("schedulers_lcm.npz")
    for name in _cases(z):
        kw = json.loads(str(z[f"{name}_kw"]))
        s = _lcm(**kw["options"])
        s.set_timesteps(**kw["set_timesteps"])
        n = len(s.timesteps)
        ref, den = z[f"{name}_traj"], z[f"{name}_denoised"]
        cut = name == "lcm_custom_strength_2"          # caller timesteps cut by strength: the reference's last step draws as well
        assert int(z[f"{name}_draws"]) == sum(s.table_impl.draws) == (n if cut else n - 1) and s.table_impl.draws[-1] == cut
        assert not cut or (n == 2 and s.timesteps.tolist() == [320, 19] and s.table_impl.num_inference_steps == 4)
        x = torch.from_numpy(ref[0])
        for i, t in enumerate(s.timesteps):
            out = s.step(g(100 + i, 1, 4, 8, 8), t, x, variance_noise=g(200 + i, 1, 4, 8, 8), return_dict=False)
            assert isinstance(out, tuple) and len(out) == 2
            x, d = out
            for got, r in ((x.numpy(), ref[i + 1]), (d.numpy(), den[i])):
                assert (np.abs(got - r) <= 2e-5 * np.abs(r) + 2e-5 * np.abs(r).max()).all(), (name, i)
        # the row mapping: the last row returns `denoised` itself and has no noise term
        c = s.table_impl.coef
        assert (c[-1, 12] == 0) == (not cut) and (c[:-1, 12] > 0).all() and (c[:, [2, 3, 4, 5, 6, 9, 10, 13, 14]] == 0).all()
        assert np.array_equal(x.numpy(), d.numpy()) == (not cut)
    r = _lcm()
    r.set_timesteps(4)
    o = r.step(g(100, 1, 4, 8, 8), r.timesteps[0], g(21, 1, 4, 8, 8), variance_noise=g(200, 1, 4, 8, 8))
    assert torch.equal(o.prev_sample, o[0]) and torch.equal(o.denoised, o[1])


def test_noise_is_drawn_in_the_reference_order():
    """n - 1 draws, after the start latents; the last slice is zero and leaves the generator where it is."""
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from blobctrl_amd.schedulers import draw_variance_noise, randn_tensor
    z = _gold("schedulers_lcm.npz")
    s = _lcm()
    s.set_timesteps(4)
    gen = torch.Generator().manual_seed(77)
    x = torch.from_numpy(z["lcm_gen77_4_traj"][0])
    for i, t in enumerate(s.timesteps):
        x = s.step(g(100 + i, 1, 4, 8, 8), t, x, generator=gen).prev_sample
        r = z["lcm_gen77_4_traj"][i + 1]
        assert (np.abs(x.numpy() - r) <= 2e-5 * np.abs(r) + 2e-5 * np.abs(r).max()).all(), i
    gen, gen2 = torch.Generator().manual_seed(77), torch.Generator().manual_seed(77)
    noise = draw_variance_noise(4, (1, 4, 8, 8), gen, "cpu", s.table_impl.draws)
    assert noise.shape == (4, 1, 4, 8, 8) and np.array_equal(noise[:3].numpy(), z["lcm_gen77_4_noise"]) and not noise[3].any()
    for _ in range(3):
        randn_tensor((1, 4, 8, 8), gen2, "cpu")
    assert torch.equal(torch.randn(3, generator=gen), torch.randn(3, generator=gen2))          # three draws were made, not four
    with pytest.raises(ValueError, match="Cannot pass both generator and variance_noise"):
        s.set_timesteps(4)
        s.step(g(100, 1, 4, 8, 8), 999, g(21, 1, 4, 8, 8), generator=gen, variance_noise=g(200, 1, 4, 8, 8))
    # the loop fixture (latents given, the generator draws the noise only) and the reference's own __call__ (start latents first)
    zl = _gold("loop_tiny_lcm.npz")
    n = BlobCtrlEngine.variance_noise(4, 1, 8, 8, torch.Generator().manual_seed(int(zl["lcm_cfg_4_seed"])), "cpu", s.table_impl.draws)
    assert np.array_equal(n[:3].numpy(), zl["lcm_cfg_4_noise"]) and not n[3].any()
    zp = _gold("pipeline_call_lcm.npz")
    gen = torch.Generator().manual_seed(int(zp["seed"]))
    randn_tensor((2, 4, 8, 8), gen, "cpu")
    n = BlobCtrlEngine.variance_noise(4, 2, 8, 8, gen, "cpu", s.table_impl.draws)
    assert np.array_equal(n[:3].numpy(), zp["cfg_noise"]) and np.array_equal(zp["cfg_noise"], zp["nocfg_noise"]) and not n[3].any()
    # a list of generators: one sample each
    gens = [torch.Generator().manual_seed(5), torch.Generator().manual_seed(6)]
    n = BlobCtrlEngine.variance_noise(2, 2, 8, 8, gens, "cpu", [True, False])
    assert torch.equal(n[0, 1:], torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(6))) and not n[1].any()


def test_refusals():
    from blobctrl_amd.schedulers import LCMScheduler, LCMTable
    for kw, word in ((dict(thresholding=True), "thresholding"), (dict(clip_sample=True), "clip_sample"),
                     (dict(prediction_type="v_prediction"), "prediction_type"), (dict(prediction_type="sample"), "prediction_type"),
                     (dict(beta_schedule="linear"), "beta_schedule"), (dict(trained_betas=[0.1, 0.2]), "trained_betas"),
                     (dict(rescale_betas_zero_snr=True), "rescale_betas_zero_snr")):
        with pytest.raises(NotImplementedError, match=word) as e:
            LCMScheduler(**kw)
        assert "not tabulated" in str(e.value), kw
    s = _lcm()
    with pytest.raises(ValueError, match="Number of inference steps"):
        s.step(g(1, 1, 4, 8, 8), 999, g(2, 1, 4, 8, 8))
    with pytest.raises(ValueError, match="exactly one"):
        s.set_timesteps()
    with pytest.raises(ValueError, match="Can only pass one"):
        s.set_timesteps(4, timesteps=[999, 500])
    with pytest.raises(ValueError, match="descending order"):
        s.set_timesteps(timesteps=[999, 500, 500])
    with pytest.raises(ValueError, match="must start before"):
        s.set_timesteps(timesteps=[1000, 500])
    with pytest.raises(ValueError, match="original_steps"):
        s.set_timesteps(4, original_inference_steps=1001)
    with pytest.raises(ValueError, match="cannot be larger than `original_inference_steps`"):
        s.set_timesteps(60, strength=1.5)
    with pytest.raises(ValueError, match="cannot be larger than `self.config.train_timesteps`"):
        s.set_timesteps(1001)
    with pytest.raises(ValueError, match="smaller than `num_inference_steps`"):
        s.set_timesteps(30, strength=0.5)
    with pytest.raises(TypeError, match="unknown LCMTable option"):
        LCMTable(use_karras_sigmas=True)


# ------------------------------------------------------------------------------------------------------------ compiled plans
@pytest.fixture(scope="module")
def dump_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("dump")


@pytest.fixture(scope="module")
def plan_dump(dump_dir):
    return build_plan_dump(dump_dir)


def _engine():
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from tests.gpu_common import tiny_trunk_configs
    usd, bsd = tiny_weights()
    ucfg, bcfg = tiny_trunk_configs()
    return BlobCtrlEngine(usd, bsd, ucfg, bcfg, device="cpu", scheduler="unipc", compile_only=True, max_cached_plans=16)


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """One compile-only engine: the LCM edit single-pass (guidance 1.0), with guidance, and on the duplicated plan; DDIM opted in; the
    third-order DPM-Solver++ table opted in."""
    from blobctrl_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, LCMScheduler
    eng = _engine()
    d = tmp_path_factory.mktemp("plans")
    lcm = LCMScheduler.from_config(DDIMScheduler().config)
    cases = {"lcm_single": (lcm, 1, dict(guidance_scale=1.0)), "lcm_cfg": (lcm, 1, dict(guidance_scale=7.5)),
             "lcm_dup": (lcm, 1, dict(guidance_scale=1.0, single_pass=False)),
             "lcm_single_b3": (lcm, 3, dict(guidance_scale=1.0)), "lcm_cfg_b3": (lcm, 3, dict(guidance_scale=7.5)),
             "lcm_custom": (lcm, 1, dict(guidance_scale=1.0, timesteps=[939, 601, 320, 19])),
             "ddim_single": (DDIMScheduler(), 1, dict(guidance_scale=1.0, single_pass=True)),
             "ddim_g1": (DDIMScheduler(), 1, dict(guidance_scale=1.0)),
             "dpm3_single": (DPMSolverMultistepScheduler(solver_order=3), 1, dict(guidance_scale=0.5, single_pass=True))}
    out = dict(eng=eng, seq={}, keys={}, plans={})
    for key, (s, B, kw) in cases.items():
        eng.set_scheduler(s.kind, s.table_params())
        out[key] = str(d / f"{key}.bcplan")
        steps = 6 if key == "dpm3_single" else 4                              # (a third-order row needs more than four steps)
        out["seq"][key] = eng.compile_plan(out[key], B, 8, 8, 7, TINY["ctx"], None if "timesteps" in kw else steps, blobnet_control_guidance_end=0.5, **kw)
        out["keys"][key] = next(reversed(eng._plans))
        out["plans"][key] = eng._plans[out["keys"][key]]
    return out


def _version(path):
    return struct.unpack("<I", open(path, "rb").read()[4:8])[0]


def test_a_guidance_free_lcm_edit_compiles_to_a_single_pass_plan(compiled, plan_dump):
    T, D = 7, TINY["ctx"]
    for single, cfg, B in (("lcm_single", "lcm_cfg", 1), ("lcm_single_b3", "lcm_cfg_b3", 3)):
        assert compiled["keys"][single][-1] == "single" and "single" not in compiled["keys"][cfg]
        assert compiled["seq"][single] == ["step_active", "step_active", "step_inactive", "step_inactive"]
        Ps, Pc = compiled["plans"][single], compiled["plans"][cfg]
        assert Ps.single and not Pc.single
        assert Ps.ctx.shape == (B, T, D) and Pc.ctx.shape == (2 * B, T, D)
        assert Ps.unet_in.shape[0] == B and Pc.unet_in.shape[0] == 2 * B and Ps.blob_in.shape == Pc.blob_in.shape
        for seg in ("prologue", "step_active", "step_inactive"):
            ms, mc = getattr(Ps, seg).meta, getattr(Pc, seg).meta
            assert [m["kind"] for m in ms] == [m["kind"] for m in mc]
            halves = same = 0
            for a, b in zip(ms, mc):
                if a["shape"] is None or a["shape"][0] not in ("dense", "conv1", "conv2", "ups"):   # (a GEMM: (variant, M, N, K, split))
                    continue
                assert a["shape"][2:4] == b["shape"][2:4], (seg, a, b)
                if seg == "prologue":                                              # prompt K / V and the UNet's time embedding: half
                    unet = a["kind"] == "ctx_kv" or (a["kind"] == "temb" and a["shape"] != b["shape"])
                else:
                    unet = a["sid"] == 0                                           # (BlobNet is recorded for the side stream)
                if unet:
                    assert 2 * a["shape"][1] == b["shape"][1], (seg, a, b)
                    halves += 1
                else:                                                              # BlobNet is what it was
                    assert a["shape"] == b["shape"], (seg, a, b)
                    same += 1
            assert halves > 10 and (same > 100) == (seg == "step_active"), (seg, halves, same)
            if seg == "prologue":
                kinds = [m["kind"] for m in ms if m["shape"] is not None and m["shape"][0] == "dense"]
                assert halves == kinds.count("ctx_kv") + 3 and same == 3 + kinds.count("collapse"), (halves, same)
        bufs, segs = plan_dump(compiled[single])
        cb, cs = plan_dump(compiled[cfg])
        sizes = {n_: b_ for n_, b_ in bufs.values() if n_ != "-"}
        csizes = {n_: b_ for n_, b_ in cb.values() if n_ != "-"}
        assert sizes["ctx"] == B * T * D * 2 and csizes["ctx"] == 2 * sizes["ctx"]
        assert {k: v for k, v in sizes.items() if k != "ctx"} == {k: v for k, v in csizes.items() if k != "ctx"}
        assert _version(compiled[single]) == 7 and _version(compiled[cfg]) == 5
        for name in ("step_active", "step_inactive"):
            ops, cops = [op for op, _, _ in segs[name]], [op for op, _, _ in cs[name]]
            assert ops[-1] == OP_STEP_SINGLE and cops[-1] == OP_STEP_NOISE and ops[:-1] == cops[:-1]
            assert OP_STEP not in ops and OP_STEP_NOISE not in ops
            op, sid, a = segs[name][-1]
            assert [_named(bufs, a[j])[0] for j in (1, 2, 3, 4, 8, 11)] == ["latents", "coef", "step_idx", "hist", "variance_noise", "eps_guided"]
            assert a[5:8] == [str(B), "8", "8"] and a[9:11] == ["4", "0"] and a[12] == "1"
            # the UNet input is assembled for B images (Bout), from B latents
            asm = [a_ for op_, sid_, a_ in segs[name] if op_ == 23 and sid_ == 0]
            casm = [a_ for op_, sid_, a_ in cs[name] if op_ == 23 and sid_ == 0]
            assert len(asm) == len(casm) == 1 and asm[0][5] == str(B) and casm[0][5] == str(2 * B) and asm[0][1] == casm[0][1] == str(B)
        # the time-embedding table of the UNet has B rows per step
        temb = [a_ for op_, _, a_ in segs["prologue"] if op_ == OP_TEMB_TABLE]
        ctemb = [a_ for op_, _, a_ in cs["prologue"] if op_ == OP_TEMB_TABLE]
        assert sorted(a_[2] for a_ in temb) == [str(B), str(B)] and sorted(a_[2] for a_ in ctemb) == sorted([str(B), str(2 * B)])
        # the stored tables: the LCM rows, the last noise coefficient 0
        coef = np.frombuffer(_stored(compiled[single])["coef"], np.float32).reshape(4, 16)
        assert coef[-1, 12] == 0 and (coef[:-1, 12] > 0).all() and (coef[:, 11] == 1).all()
        assert np.frombuffer(_stored(compiled[single])["t_table"], np.float32).tolist() == [999, 759, 499, 259]
    assert np.frombuffer(_stored(compiled["lcm_custom"])["t_table"], np.float32).tolist() == [939, 601, 320, 19]
    assert compiled["keys"]["lcm_custom"] == compiled["keys"]["lcm_single"]           # other timesteps: the same plan


def test_single_pass_is_the_default_for_lcm_only(compiled, plan_dump, tmp_path):
    keys = compiled["keys"]
    assert "single" not in keys["lcm_dup"] and keys["lcm_dup"] == keys["lcm_cfg"]       # single_pass=False: the duplicated plan
    assert "single" not in keys["ddim_g1"] and _version(compiled["ddim_g1"]) == 5       # guidance off, DDIM: the plan it always had
    assert keys["ddim_single"][-1] == "single" and _version(compiled["ddim_single"]) == 7
    for key, third, noise in (("ddim_single", "0", False), ("dpm3_single", "1", False), ("lcm_single", "0", True)):
        bufs, segs = plan_dump(compiled[key])
        op, _, a = segs["step_inactive"][-1]
        assert op == OP_STEP_SINGLE and a[10] == third and (a[8] != "p-") == noise, key
    eng = compiled["eng"]
    from blobctrl_amd.schedulers import LCMScheduler
    s = LCMScheduler()
    eng.set_scheduler(s.kind, s.table_params())
    with pytest.raises(ValueError, match="single_pass"):
        eng.compile_plan(str(tmp_path / "x.bcplan"), 1, 8, 8, 7, TINY["ctx"], 4, guidance_scale=7.5, single_pass=True)
    with pytest.raises(NotImplementedError, match="eta"):
        eng.compile_plan(str(tmp_path / "x.bcplan"), 1, 8, 8, 7, TINY["ctx"], 4, eta=0.5)
    with pytest.raises(ValueError, match="variance_noise"):
        eng.compile_plan(str(tmp_path / "x.bcplan"), 1, 8, 8, 7, TINY["ctx"], 4, variance_noise=torch.zeros(3, 1, 4, 8, 8))
    assert not os.path.exists(tmp_path / "x.bcplan")
    eng.set_scheduler("unipc")
    with pytest.raises(NotImplementedError, match="timesteps"):
        eng.compile_plan(str(tmp_path / "x.bcplan"), 1, 8, 8, 7, TINY["ctx"], 4, timesteps=[999, 500, 10])
    with pytest.raises(NotImplementedError, match="coefficient table"):
        eng.set_scheduler("tcd")


def test_split_cfg_is_ignored_on_a_single_pass_plan(monkeypatch):
    monkeypatch.setenv("BC_SPLIT_CFG", "1")
    eng = _engine()
    P = eng.plan_for(1, 8, 8, 7, TINY["ctx"], 4, stochastic=True, single=True)
    assert P.single and not P.split_cfg and P.ctx.shape[0] == 1
    assert eng.plan_for(1, 8, 8, 7, TINY["ctx"], 4, stochastic=True).split_cfg


def test_a_version_6_file_cannot_carry_the_single_pass_step(compiled, plan_dump, tmp_path):
    raw = bytearray(open(compiled["lcm_single"], "rb").read())
    plan_dump(compiled["lcm_single"])                                          # the version-7 file itself loads
    for v in (5, 6):
        raw[4:8] = struct.pack("<I", v)
        bad = tmp_path / f"v{v}.bcplan"
        bad.write_bytes(bytes(raw))
        with pytest.raises(AssertionError, match="unknown op"):
            plan_dump(str(bad))
    raw[4:8] = struct.pack("<I", 8)
    (tmp_path / "v8.bcplan").write_bytes(bytes(raw))
    with pytest.raises(AssertionError, match="unsupported plan version"):
        plan_dump(str(tmp_path / "v8.bcplan"))


def test_existing_configurations_compile_to_the_listings_they_had(plan_dump, dump_dir, tmp_path):
    """UniPC, DDIM, stochastic DDIM, DPM-Solver++ 3M, SDE-DPM-Solver++, Euler and Heun at the geometry of tests/test_euler_cpu.py: the
    file version and the whole launch listing (every non-GEMM launch with its arguments, every buffer with its size) are those the
    commit before the LCM scheduler wrote."""
    from blobctrl_amd.schedulers import (DDIMScheduler, DPMSolverMultistepScheduler, EulerDiscreteScheduler, HeunDiscreteScheduler,
                                         UniPCMultistepScheduler)
    want = json.load(open(os.path.join(GOLD, "plan_listings_before_lcm.json")))
    eng = _engine()
    n, B, h, w, T = 6, 1, 8, 8, 7
    noise = g(5, n, B, 4, h, w)
    scheds = {"uni": (UniPCMultistepScheduler(), {}), "ddim": (DDIMScheduler(), {}),
              "ddim_eta": (DDIMScheduler(), dict(eta=1.0, variance_noise=noise)),
              "dpm3": (DPMSolverMultistepScheduler(solver_order=3), {}),
              "sde": (DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++"), dict(variance_noise=noise)),
              "euler": (EulerDiscreteScheduler(**SD), {}), "heun": (HeunDiscreteScheduler(**SD), {})}
    assert sorted(scheds) == sorted(want)
    for key, (s, kw) in scheds.items():
        eng.set_scheduler(s.kind, s.table_params())
        path = str(tmp_path / f"{key}.bcplan")
        eng.compile_plan(path, B, h, w, T, TINY["ctx"], n, blobnet_control_guidance_end=0.67, **kw)
        assert _version(path) == want[key]["version"], key
        r = subprocess.run([os.path.join(str(dump_dir), "plan_dump"), path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
        assert len(r.stdout.splitlines()) == want[key]["lines"], key
        assert hashlib.sha256(r.stdout.encode()).hexdigest() == want[key]["sha256"], key


def test_new_entry_points_are_exported_beside_the_old_ones():
    from blobctrl_amd import _lib
    lib = _lib.load()
    old = ("bc_cfg_scheduler_step", "bc_cfg_scheduler_step_noise", "bc_cfg_scheduler_step3", "bc_timestep_embedding",
           "bc_timestep_embedding_table", "bc_assemble_input", "bc_assemble_input_im2col", "bc_assemble_input_scaled",
           "bc_assemble_input_im2col_scaled")
    for name in old + ("bc_scheduler_step_single",):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert _lib.OPS["bc_scheduler_step_single"] == OP_STEP_SINGLE and _lib.op_signature("bc_scheduler_step_single") == "pppppiiipiipi"
    assert [_lib.OPS[k] for k in ("bc_cfg_scheduler_step", "bc_cfg_scheduler_step_noise", "bc_cfg_scheduler_step3")] == [11, 30, 31]


# ------------------------------------------------------------------------------------------------------------ time_cond_proj_dim
COND_DIM = 8


def _cond_unet():
    """(state dict, TrunkConfig) of the tiny UNet with time_cond_proj_dim = 8: the plain tiny UNet plus time_embedding.cond_proj.weight."""
    import dataclasses
    from blobctrl_amd import synth
    from tests.gpu_common import tiny_trunk_configs
    c = TINY
    shapes = synth.trunk_param_shapes(5, c["boc"], 2, c["ctx"], 4, blobnet=False, time_cond_proj_dim=COND_DIM)
    return synth.synth_state_dict(shapes, c["seed"]), dataclasses.replace(tiny_trunk_configs()[0], time_cond_proj_dim=COND_DIM)


def test_guidance_scale_embedding_equals_the_reference_bit_for_bit():
    from blobctrl_amd.pipeline import get_guidance_scale_embedding
    z = _gold("unet_tiny_timecond.npz")
    scales = z["scales"].tolist()
    assert scales == [1.0, 3.0, 7.5]
    for dim in (8, 7, 256):
        ref = z[f"embedding_{dim}"]
        got = get_guidance_scale_embedding(torch.tensor([s - 1 for s in scales], dtype=torch.float32), embedding_dim=dim)
        assert got.dtype == torch.float32 and got.shape == (3, dim) and np.array_equal(got.numpy(), ref), dim
        for i, s in enumerate(scales):                                  # as pipe:990 builds its argument
            one = get_guidance_scale_embedding(torch.tensor(s - 1).repeat(2), dim)
            assert np.array_equal(one.numpy(), np.stack([ref[i], ref[i]])), (dim, s)
    assert (z["embedding_7"][:, -1] == 0).all() and (z["embedding_8"][0] == [0, 0, 0, 0, 1, 1, 1, 1]).all()
    with pytest.raises(ValueError):
        get_guidance_scale_embedding(torch.zeros(2, 2))


def test_schema_and_loader_know_cond_proj(tmp_path):
    from blobctrl_amd import checkpoint as ck, synth
    from blobctrl_amd.weights import PackedTrunk, merge_lora
    c = TINY
    usd, ucfg = _cond_unet()
    plain = tiny_weights()[0]
    assert [k for k in usd if k not in plain] == ["time_embedding.cond_proj.weight"] and all(torch.equal(usd[k], plain[k]) for k in plain)
    assert tuple(usd["time_embedding.cond_proj.weight"].shape) == (c["boc"][0], COND_DIM)
    assert "time_embedding.cond_proj.weight" not in synth.trunk_param_shapes(4 + 1 + c["feat"], c["boc"], 2, None, None, blobnet=True)
    full = synth.trunk_param_shapes(5, (320, 640, 1280, 1280), 2, 768, 4, blobnet=False, time_cond_proj_dim=256)
    assert full["time_embedding.cond_proj.weight"] == (320, 256)
    pw = PackedTrunk(usd, "cpu", c["boc"])
    assert torch.equal(pw.h["time_embedding.cond_proj.weight"], usd["time_embedding.cond_proj.weight"].half())
    # a LoRA that does not name it leaves it alone
    wq = "down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q"
    cp = "time_embedding.cond_proj"
    lora = {f"{wq}.lora_A.weight": g(1, 4, c["boc"][0]) * 0.2, f"{wq}.lora_B.weight": g(2, c["boc"][0], 4) * 0.2}
    merged = merge_lora(usd, lora, {wq: 4.0})
    assert torch.equal(merged[cp + ".weight"], usd[cp + ".weight"]) and not torch.equal(merged[wq + ".weight"], usd[wq + ".weight"])
    # ... and one that names it is merged into it like into any linear layer
    lora = {f"{cp}.lora_A.weight": g(3, 2, COND_DIM) * 0.2, f"{cp}.lora_B.weight": g(4, c["boc"][0], 2) * 0.2}
    merged = merge_lora(usd, lora, {cp: 2.0})
    assert torch.allclose(merged[cp + ".weight"], usd[cp + ".weight"] + lora[f"{cp}.lora_B.weight"] @ lora[f"{cp}.lora_A.weight"])
    # config.json -> TrunkConfig / ModelConfig; a config and a checkpoint that disagree are refused
    d = tmp_path / "unet"
    d.mkdir()
    cfg = {"block_out_channels": list(c["boc"]), "attention_head_dim": c["heads"], "norm_num_groups": c["groups"], "in_channels": 5,
           "cross_attention_dim": c["ctx"], "time_cond_proj_dim": COND_DIM}
    ck.write_safetensors(str(d / "diffusion_pytorch_model.safetensors"), usd)
    json.dump(cfg, open(d / "config.json", "w"))
    sd, tc = ck.load_unet(str(d), extra_in_channels=0)
    assert tc.time_cond_proj_dim == COND_DIM and tc == ucfg and torch.equal(sd["time_embedding.cond_proj.weight"], usd["time_embedding.cond_proj.weight"])
    json.dump(dict(cfg, time_cond_proj_dim=None), open(d / "config.json", "w"))
    with pytest.raises(ValueError, match="time_cond_proj_dim"):
        ck.load_unet(str(d), extra_in_channels=0)
    ck.write_safetensors(str(d / "diffusion_pytorch_model.safetensors"), plain)
    assert ck.load_unet(str(d), extra_in_channels=0)[1].time_cond_proj_dim is None
    json.dump(cfg, open(d / "config.json", "w"))
    with pytest.raises(ValueError, match="time_cond_proj_dim"):
        ck.load_unet(str(d), extra_in_channels=0)
    from blobctrl_amd.modules import UNet2DConditionModel
    json.dump(cfg, open(d / "config.json", "w"))
    ck.write_safetensors(str(d / "diffusion_pytorch_model.safetensors"), usd)
    m = UNet2DConditionModel.from_pretrained(str(tmp_path), subfolder="unet", device="cpu")
    assert m.config.time_cond_proj_dim == COND_DIM and m.config["time_cond_proj_dim"] == COND_DIM


def test_a_time_cond_unet_compiles_the_cond_embedding_and_runs_single_pass(plan_dump, tmp_path):
    """pipe:497: a UNet with time_cond_proj_dim never runs classifier-free guidance, whatever the scale - the scale goes in through the
    named buffer `timestep_cond`, replay-time data of the plan.  The prologue holds cond_proj as one GEMM and the `_cond` time-embedding
    table for the UNet; BlobNet's table is the plain one."""
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from blobctrl_amd.schedulers import DDIMScheduler, LCMScheduler, UniPCMultistepScheduler
    from tests.gpu_common import tiny_trunk_configs
    usd, ucfg = _cond_unet()
    eng = BlobCtrlEngine(usd, tiny_weights()[1], ucfg, tiny_trunk_configs()[1], device="cpu", scheduler="unipc", compile_only=True,
                         max_cached_plans=8)
    B, T = 2, 7
    for sched, single_pass, Bu in ((LCMScheduler.from_config(DDIMScheduler().config), None, B), (UniPCMultistepScheduler(), None, B),
                                   (UniPCMultistepScheduler(), False, 2 * B)):
        eng.set_scheduler(sched.kind, sched.table_params())
        path = str(tmp_path / f"{sched.kind}_{Bu}.bcplan")
        eng.compile_plan(path, B, 8, 8, T, TINY["ctx"], 4, guidance_scale=7.5, blobnet_control_guidance_end=0.5, single_pass=single_pass)
        key = next(reversed(eng._plans))
        P = eng._plans[key]
        assert (key[-1] == "single") == (Bu == B) and P.single == (Bu == B) and P.ctx.shape[0] == Bu
        assert P.timestep_cond.shape == (Bu, COND_DIM) and P.timestep_cond.dtype == torch.float16
        assert _version(path) == 7
        bufs, segs = plan_dump(path)
        sizes = {n_: b_ for n_, b_ in bufs.values() if n_ != "-"}
        assert sizes["timestep_cond"] == Bu * COND_DIM * 2 and "timestep_cond" not in _stored(path)
        tables = [(op, a) for op, _, a in segs["prologue"] if op in (OP_TEMB_TABLE, 35)]
        assert sorted(op for op, _ in tables) == [OP_TEMB_TABLE, 35]
        for op, a in tables:
            assert a[1:4] == ["4", str(Bu if op == 35 else B), str(TINY["boc"][0])] and _named(bufs, a[0]) == ("t_table", 0)
        assert not any(op in (35, 36, 9) for name in ("step_active", "step_inactive") for op, _, _ in segs[name])
        gemms = [m["shape"] for m in P.prologue.meta if m["kind"] == "temb" and m["shape"] is not None and m["shape"][0] == "dense"]
        assert ("dense", Bu, TINY["boc"][0], COND_DIM, 1) in gemms and len(gemms) == 7
    # a plain UNet has no such buffer and no such op; a timestep_cond for it is refused (test_lcm_gpu.py: the module shell and denoise)
    eng2 = _engine()
    P = eng2.plan_for(1, 8, 8, 7, TINY["ctx"], 4)
    assert P.timestep_cond is None and all(m["shape"] != ("dense", 2, TINY["boc"][0], COND_DIM, 1) for m in P.prologue.meta)


def test_cond_entry_points_are_exported():
    from blobctrl_amd import _lib
    lib = _lib.load()
    assert _lib.OPS["bc_timestep_embedding_table_cond"] == 35 and _lib.OPS["bc_timestep_embedding_cond"] == 36
    assert _lib.op_signature("bc_timestep_embedding_table_cond") == "piiipp" and _lib.op_signature("bc_timestep_embedding_cond") == "ppfiipp"
    assert lib.bc_timestep_embedding_table_cond is not None and lib.bc_timestep_embedding_cond is not None
    assert _lib.OPS["bc_timestep_embedding"] == 9 and _lib.OPS["bc_timestep_embedding_table"] == 10
