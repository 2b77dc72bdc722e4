"""Euler, Euler-ancestral and Heun without a GPU: the coefficient tables and the drop-in schedulers against the reference's
EulerDiscreteScheduler / EulerAncestralDiscreteScheduler / HeunDiscreteScheduler (tests/golden/schedulers_euler.npz, euler_config.json),
the noise the reference drew (loop_tiny_euler.npz, pipeline_call_euler.npz), every refusal, and what compiled plans launch: the
`_scaled` input assemblies for these schedulers and for no other (read back through the host-side `.bcplan` parser)."""
import json
import os
import struct

import numpy as np
import pytest
import torch

from tests.common import TINY, build_plan_dump, g, plan_named as _named, plan_stored as _stored, tiny_weights

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
OP_ASSEMBLE, OP_IM2COL, OP_ASSEMBLE_SCALED, OP_IM2COL_SCALED = 8, 23, 32, 33
OP_STEP, OP_STEP_NOISE = 11, 30
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000, steps_offset=1)


def _gold(name):
    return np.load(os.path.join(GOLD, name))


def _cases():
    z = _gold("schedulers_euler.npz")
    return sorted(k[:-3] for k in z.files if k.endswith("_kw"))


def _case_kw(z, name):
    kw = json.loads(str(z[f"{name}_kw"]))
    return kw.pop("cls"), kw.pop("n"), kw.pop("timesteps"), kw


def _scheduler(cls, **kw):
    from blobctrl_amd import schedulers
    return {"euler": schedulers.EulerDiscreteScheduler, "euler_ancestral": schedulers.EulerAncestralDiscreteScheduler,
            "heun": schedulers.HeunDiscreteScheduler}[cls](**dict(SD, **kw))


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


def _check_traj(got, ref, what):
    assert got.shape == ref.shape, what
    for i in range(1, ref.shape[0]):                         # the bar of test_dpm_solver_cpu.py (test_host_cpu.py:98), per step
        err = np.abs(got[i] - ref[i]).max()
        assert err <= 5e-6 * np.abs(ref[i]).max(), (what, i, err)


def test_the_fixture_holds_the_cases_the_tables_are_specified_on():
    names = set(_cases())
    assert {"euler_leading_5", "euler_leading_20", "euler_leading_50", "euler_linspace_15", "euler_trailing_karras_10", "euler_sigmamin_8",
            "euler_custom_10", "eulera_noise_15", "heun_10", "heun_karras_6"} <= names
    files = set(_gold("schedulers_euler.npz").files)
    for name in names | {"eulera_gen77_5"}:                         # every case holds the whole set
        assert {f"{name}_{k}" for k in ("timesteps", "sigmas", "init_noise_sigma", "scaled", "traj")} <= files, name


@pytest.mark.parametrize("name", _cases())
def test_table_rows_reproduce_the_reference(name):
    """Timesteps, sigmas, init_noise_sigma and scale_model_input bit for bit; the trajectory through the table rows."""
    from blobctrl_amd.schedulers import apply_table_step, table_class
    z = _gold("schedulers_euler.npz")
    cls, n, ts, kw = _case_kw(z, name)
    Table = table_class(cls)
    opts = {k: v for k, v in dict(SD, **kw).items() if k != "beta_schedule" and (k != "steps_offset" or k in Table._option_defaults)}
    tab = Table(**opts)
    assert tab.init_noise_sigma > 14.6                              # (of the training sigmas: read it again after set_timesteps)
    tab.set_timesteps(timesteps=ts) if ts is not None else tab.set_timesteps(n)
    ref_t, ref_s = z[f"{name}_timesteps"], z[f"{name}_sigmas"]
    assert _same_timesteps(tab.timesteps.numpy(), ref_t, kw.get("use_karras_sigmas"))
    assert tab.sigmas.dtype == torch.float32 and np.array_equal(tab.sigmas.numpy(), ref_s)
    assert tab.init_noise_sigma == float(z[f"{name}_init_noise_sigma"]) and tab.init_noise_sigma > 1.0
    evals = len(ref_t)
    assert tab.scales_input and tab.coef.shape == (evals, 16) and torch.isfinite(tab.coef).all()
    assert evals == (2 * n - 1 if cls == "heun" else (n if ts is None else len(ts))) and tab.order == (2 if cls == "heun" else 1)
    # column 14 is the input divisor of the step's own sigma; column 11 (guidance) and 15 stay free
    assert torch.equal(tab.coef[:, 14], (tab.sigmas[:evals] ** 2 + 1) ** 0.5) and (tab.coef[:, 14] > 1).all()
    assert (tab.coef[:, 11] == 0).all() and (tab.coef[:, 15] == 0).all() and (tab.coef[:, 13] == 0).all()
    assert bool((tab.coef[:, 12] != 0).any()) == (cls == "euler_ancestral") == bool(getattr(tab, "sde", False))
    assert bool((tab.coef[:, 2] != 0).any()) == (cls == "heun")
    if cls == "heun":                                               # first stages (even rows) leave the history alone, second stages read it
        assert (tab.coef[0::2, 2] == 0).all() and (tab.coef[1::2, 2] == 1).all() and (tab.coef[1::2, 5:7] == 0).all()
    fixed = g(22, 1, 4, 8, 8)
    for i in range(evals):                                          # the same fp32 division as the reference's scale_model_input
        assert np.array_equal((fixed / tab.coef[i, 14]).numpy(), z[f"{name}_scaled"][i]), (name, i)
    ref = z[f"{name}_traj"]
    x = torch.from_numpy(ref[0])
    assert np.array_equal((g(21, 1, 4, 8, 8) * tab.init_noise_sigma).numpy(), ref[0])
    zz = torch.zeros_like(x)
    hist = dict(m0=zz, m1=zz.clone(), last=zz.clone())
    xs = [x]
    for i in range(evals):
        noise = g(200 + i, 1, 4, 8, 8) if cls == "euler_ancestral" else None
        x = apply_table_step(tab.coef[i].tolist(), g(100 + i, 1, 4, 8, 8), x, hist, noise)
        xs.append(x)
    _check_traj(torch.stack(xs).numpy(), ref, name)


def test_existing_tables_leave_column_14_at_zero_and_do_not_scale():
    from blobctrl_amd.schedulers import DDIMTable, DPMSolverMultistepTable, TableScheduler, UniPCTable
    for tab in (UniPCTable().set_timesteps(20), DDIMTable().set_timesteps(20), DDIMTable().set_timesteps(20, eta=1.0),
                DPMSolverMultistepTable(solver_order=3).set_timesteps(20), DPMSolverMultistepTable(algorithm_type="sde-dpmsolver++").set_timesteps(20)):
        assert (tab.coef[:, 14] == 0).all() and not tab.scales_input and tab.init_noise_sigma == 1.0
    x = g(3, 1, 4, 8, 8)
    for kind in ("unipc", "ddim", "dpmsolver"):
        s = TableScheduler(kind)
        s.set_timesteps(5)
        assert s.scale_model_input(x, s.timesteps[0]) is x


def _run(s, kw_of_step, n=None, ts=None):
    s.set_timesteps(timesteps=ts) if ts is not None else s.set_timesteps(n)
    fixed = g(22, 1, 4, 8, 8)
    x = g(21, 1, 4, 8, 8) * s.init_noise_sigma
    xs, scaled = [x], []
    for i, t in enumerate(s.timesteps):
        scaled.append(s.scale_model_input(fixed, t))
        out = s.step(g(100 + i, 1, 4, 8, 8), t, x, **kw_of_step(i))
        x = out[0] if type(out) is tuple else out.prev_sample
        xs.append(x)
    return torch.stack(xs).numpy(), torch.stack(scaled).numpy()


@pytest.mark.parametrize("name", _cases())
def test_dropin_schedulers_reproduce_the_reference(name):
    z = _gold("schedulers_euler.npz")
    cls, n, ts, kw = _case_kw(z, name)
    s = _scheduler(cls, **kw)
    noise = (lambda i: dict(variance_noise=g(200 + i, 1, 4, 8, 8))) if cls == "euler_ancestral" else (lambda i: {})
    got, scaled = _run(s, lambda i: dict(noise(i), return_dict=(i % 2 == 0)), n, ts)
    assert _same_timesteps(s.timesteps.numpy(), z[f"{name}_timesteps"], kw.get("use_karras_sigmas")) and \
        np.array_equal(s.sigmas.numpy(), z[f"{name}_sigmas"])
    assert s.init_noise_sigma == float(z[f"{name}_init_noise_sigma"]) and s.order == (2 if cls == "heun" else 1)
    assert s.num_inference_steps == (n if ts is None else len(ts))
    assert np.array_equal(scaled, z[f"{name}_scaled"])
    _check_traj(got, z[f"{name}_traj"], name)


def test_ancestral_generator_draws_what_the_reference_drew():
    z = _gold("schedulers_euler.npz")
    gen = torch.Generator().manual_seed(77)
    s = _scheduler("euler_ancestral")
    got, scaled = _run(s, lambda i: dict(generator=gen), 5)
    assert np.array_equal(s.timesteps.numpy(), z["eulera_gen77_5_timesteps"]) and np.array_equal(s.sigmas.numpy(), z["eulera_gen77_5_sigmas"])
    assert s.init_noise_sigma == float(z["eulera_gen77_5_init_noise_sigma"]) and np.array_equal(scaled, z["eulera_gen77_5_scaled"])
    _check_traj(got, z["eulera_gen77_5_traj"], "generator")
    assert np.abs(got[1:] - z["eulera_noise_15_traj"][1:6]).max() > 1e-2          # (other noise: really another trajectory)
    with pytest.raises(ValueError, match="variance_noise"):
        s = _scheduler("euler_ancestral")
        s.set_timesteps(5)
        s.step(g(1, 1, 4, 8, 8), s.timesteps[0], g(2, 1, 4, 8, 8), generator=gen, variance_noise=g(3, 1, 4, 8, 8))
    # Euler draws and discards one tensor per step when it is given a generator, as the reference does: the generator moves on
    s = _scheduler("euler")
    s.set_timesteps(3)
    a, b = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    s.step(g(1, 1, 4, 8, 8), s.timesteps[0], g(2, 1, 4, 8, 8), generator=a)
    torch.randn(1, 4, 8, 8, generator=b)
    assert torch.equal(torch.randn(4, generator=a), torch.randn(4, generator=b))


def test_noise_helper_draws_what_the_reference_drew():
    from blobctrl_amd.pipeline import BlobCtrlEngine
    z = _gold("loop_tiny_euler.npz")
    ref = z["eulera_5_noise"]
    got = BlobCtrlEngine.variance_noise(ref.shape[0], 1, 8, 8, torch.Generator().manual_seed(int(z["eulera_5_seed"])), device="cpu")
    assert np.array_equal(got.numpy(), ref)
    zc = _gold("pipeline_call_euler.npz")                           # __call__: the start latents first, then every step's noise
    gen = torch.Generator().manual_seed(int(zc["seed"]))
    B = zc["eulera_latents"].shape[0]
    torch.randn((B, 4, 8, 8), generator=gen, dtype=torch.float32)
    got = BlobCtrlEngine.variance_noise(int(zc["num_inference_steps"]), B, 8, 8, gen, device="cpu")
    assert np.array_equal(got.numpy(), zc["eulera_noise"])


# ------------------------------------------------------------------------------------------------------------------ configuration
@pytest.mark.parametrize("cls", ["euler", "euler_ancestral", "heun"])
def test_dropin_config_matches_the_reference(cls, tmp_path):
    from blobctrl_amd import schedulers
    from blobctrl_amd.schedulers import DPMSolverMultistepScheduler, PNDMScheduler, UniPCMultistepScheduler, scheduler_from_config_dir
    ref = json.load(open(os.path.join(GOLD, "euler_config.json")))
    Cls = type(_scheduler(cls))
    s = Cls.from_config(ref["source"])
    cfg = dict(s.config)
    cfg["_use_default_values"] = sorted(cfg["_use_default_values"])
    assert cfg == ref[cls]
    # through the PNDM configuration holder the scripts start from, and through a UniPC / DPM scheduler built from it
    p = PNDMScheduler(**{k: v for k, v in ref["source"].items() if not k.startswith("_") and k != "trained_betas"})
    for src in (p, UniPCMultistepScheduler.from_config(p.config), DPMSolverMultistepScheduler.from_config(p.config)):
        s2 = Cls.from_config(src.config)
        for k in set(Cls._defaults) | {"beta_start", "beta_end", "num_train_timesteps", "steps_offset", "beta_schedule", "prediction_type"}:
            assert s2.config[k] == ref[cls][k], (type(src).__name__, k)
        assert s2.config.steps_offset == 1 and s2.kind == cls
    s2 = Cls.from_config(p.config)
    assert s2.config.timestep_spacing == "linspace"                 # SD-1.5's scheduler_config.json has none: PNDM's default does not travel
    s2.set_timesteps(5)
    assert s2.timesteps.tolist() == ([999.0, 749.25, 499.5, 249.75, 0.0] if cls != "heun" else
                                     [999.0, 749.25, 749.25, 499.5, 499.5, 249.75, 249.75, 0.0, 0.0])
    assert abs(s2.init_noise_sigma - 14.6146) < 1e-3
    import copy
    copy.deepcopy(s2)
    k = Cls.from_config(p.config, timestep_spacing="trailing")
    assert k.config.timestep_spacing == "trailing" and "timestep_spacing" not in k.config._use_default_values
    assert k.table_params()[:3] == (1000, 0.00085, 0.012) and ("timestep_spacing", "trailing") in k.table_params()[3]
    # <model>/scheduler/scheduler_config.json naming the class
    with open(tmp_path / "scheduler_config.json", "w") as f:
        json.dump(dict(ref["source"], _class_name=Cls.__name__), f)
    got = scheduler_from_config_dir(str(tmp_path))
    assert type(got) is Cls and got.config.steps_offset == 1 and schedulers.table_class(got.kind) is type(got.table_impl)


def test_refused_options_name_the_option():
    from blobctrl_amd.schedulers import (EulerAncestralDiscreteScheduler, EulerDiscreteScheduler, EulerDiscreteTable, HeunDiscreteScheduler)
    x = torch.zeros(1, 4, 8, 8)
    for Cls, kw, word in ((EulerDiscreteScheduler, dict(prediction_type="v_prediction"), "prediction_type"),
                          (EulerDiscreteScheduler, dict(prediction_type="sample"), "prediction_type"),
                          (EulerDiscreteScheduler, dict(interpolation_type="log_linear"), "interpolation_type"),
                          (EulerDiscreteScheduler, dict(timestep_type="continuous"), "timestep_type"),
                          (EulerDiscreteScheduler, dict(rescale_betas_zero_snr=True), "rescale_betas_zero_snr"),
                          (EulerDiscreteScheduler, dict(sigma_min=0.1), "sigma_min"),
                          (EulerDiscreteScheduler, dict(trained_betas=[0.1, 0.2]), "trained_betas"),
                          (EulerDiscreteScheduler, dict(beta_schedule="linear"), "beta_schedule"),
                          (EulerAncestralDiscreteScheduler, dict(prediction_type="v_prediction"), "prediction_type"),
                          (EulerAncestralDiscreteScheduler, dict(rescale_betas_zero_snr=True), "rescale_betas_zero_snr"),
                          (EulerAncestralDiscreteScheduler, dict(trained_betas=[0.1]), "trained_betas"),
                          (HeunDiscreteScheduler, dict(prediction_type="v_prediction"), "prediction_type"),
                          (HeunDiscreteScheduler, dict(clip_sample=True), "clip_sample"),
                          (HeunDiscreteScheduler, dict(trained_betas=[0.1]), "trained_betas"),
                          (HeunDiscreteScheduler, dict(beta_schedule="exp"), "beta_schedule")):
        with pytest.raises(NotImplementedError, match=word):
            Cls(**kw)
    for kw, word in ((dict(interpolation_type="log_linear"), "interpolation_type"), (dict(timestep_type="continuous"), "timestep_type")):
        with pytest.raises(NotImplementedError, match=word):
            EulerDiscreteTable(**kw)
    s = EulerDiscreteScheduler()
    with pytest.raises(NotImplementedError, match="sigmas"):
        s.set_timesteps(sigmas=[14.0, 1.0, 0.0])
    with pytest.raises(ValueError, match="exactly one"):
        s.set_timesteps()
    with pytest.raises(ValueError, match="Can only pass one"):
        s.set_timesteps(10, timesteps=[999, 500])
    with pytest.raises(ValueError, match="use_karras_sigmas"):
        EulerDiscreteScheduler(use_karras_sigmas=True).set_timesteps(timesteps=[999, 500])
    with pytest.raises(ValueError, match="final_sigmas_type"):
        EulerDiscreteScheduler(final_sigmas_type="nope").set_timesteps(10)
    with pytest.raises(ValueError, match="is not supported"):
        EulerDiscreteScheduler(timestep_spacing="nope").set_timesteps(10)
    with pytest.raises(ValueError, match="Number of inference steps"):
        EulerDiscreteScheduler().step(x, 999.0, x)
    s.set_timesteps(5)
    with pytest.raises(NotImplementedError, match="s_churn"):
        s.step(x, s.timesteps[0], x, s_churn=0.5)
    with pytest.raises(NotImplementedError, match="timesteps"):
        HeunDiscreteScheduler().set_timesteps(timesteps=[999, 500])
    with pytest.raises(TypeError):                                  # the reference's set_timesteps takes none
        EulerAncestralDiscreteScheduler().set_timesteps(timesteps=[999, 500])


# ------------------------------------------------------------------------------------------------------------------ engine tables
def _bare_engine():
    from blobctrl_amd.pipeline import BlobCtrlEngine
    eng = BlobCtrlEngine.__new__(BlobCtrlEngine)
    eng._sched_cache, eng.scheduler_kind, eng.scheduler_params = {}, "unipc", (1000, 0.00085, 0.012)
    return eng


def test_engine_tables_follow_the_scheduler_objects():
    eng = _bare_engine()
    for cls, kw, n in (("euler", dict(use_karras_sigmas=True), 6), ("euler", dict(timestep_spacing="leading"), 20),
                       ("euler_ancestral", dict(timestep_spacing="trailing"), 7), ("heun", dict(use_karras_sigmas=True), 4)):
        s = _scheduler(cls, **kw)
        eng.set_scheduler(s.kind, s.table_params())
        tab = eng._scheduler_table(n)
        s.set_timesteps(n)
        assert torch.equal(tab.table(), s.table_impl.table()) and torch.equal(tab.timesteps, s.timesteps), cls
        assert tab.init_noise_sigma == s.init_noise_sigma and tab.scales_input
        assert eng._step_form(tab, False) == (cls == "euler_ancestral", False)
        assert len(tab.timesteps) == (2 * n - 1 if cls == "heun" else n)
    # caller timesteps: Euler takes them (fractional ones too: nothing rounds them), the other two refuse
    s = _scheduler("euler")
    eng.set_scheduler(s.kind, s.table_params())
    ts = [999, 850.5, 700.25, 20]
    tab = eng._scheduler_table(len(ts), timesteps=ts)
    assert tab.timesteps.tolist() == ts and tab.timesteps.dtype == torch.float32
    for cls in ("euler_ancestral", "heun"):
        s = _scheduler(cls)
        eng.set_scheduler(s.kind, s.table_params())
        with pytest.raises(NotImplementedError, match="timesteps"):
            eng._scheduler_table(4, timesteps=[999, 700, 400, 20])
        eng.scheduler_kind = cls
        with pytest.raises(NotImplementedError, match="eta"):
            eng._check_eta(0.5)
    with pytest.raises(NotImplementedError, match="coefficient table"):
        eng.set_scheduler("lms")


# ------------------------------------------------------------------------------------------------------------ compiled plans
@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    return build_plan_dump(tmp_path_factory.mktemp("dump"))


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """One compile-only engine; plans of UniPC, DDIM, stochastic DDIM, DPM-Solver++ and the three new schedulers at the same geometry."""
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from blobctrl_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler
    from tests.gpu_common import tiny_trunk_configs
    usd, bsd = tiny_weights()
    ucfg, bcfg = tiny_trunk_configs()
    eng = BlobCtrlEngine(usd, bsd, ucfg, bcfg, device="cpu", scheduler="unipc", compile_only=True, max_cached_plans=8)
    d = tmp_path_factory.mktemp("plans")
    n, B, h, w, T = 6, 1, 8, 8, 7
    noise = g(5, n, B, 4, h, w)
    scheds = {"uni": (UniPCMultistepScheduler(), {}), "ddim": (DDIMScheduler(), {}), "ddim_eta": (DDIMScheduler(), dict(eta=1.0)),
              "dpm": (DPMSolverMultistepScheduler(use_karras_sigmas=True), {}), "dpm3": (DPMSolverMultistepScheduler(solver_order=3), {}),
              "sde": (DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++"), {}),
              "euler": (_scheduler("euler", timestep_spacing="leading"), {}),
              "euler_custom": (_scheduler("euler"), dict(timesteps=[999, 850.5, 700, 550, 400, 20])),
              "eulera": (_scheduler("euler_ancestral"), dict(variance_noise=noise)),
              "heun": (_scheduler("heun"), {})}
    out = dict(n=n, noise=noise, seq={}, scheds=scheds, stats={})
    for key, (s, kw) in scheds.items():
        eng.set_scheduler(s.kind, s.table_params())
        out[key] = str(d / f"{key}.bcplan")
        out["seq"][key] = eng.compile_plan(out[key], B, h, w, T, TINY["ctx"], n, blobnet_control_guidance_end=0.67, **kw)
        out["stats"][key] = dict(eng.cache_stats)
    return out


def test_compiled_plans_of_the_new_schedulers_assemble_scaled_inputs(compiled, plan_dump):
    n = compiled["n"]
    ub, us = plan_dump(compiled["uni"])
    uni_asm = {name: [(i, op) for i, (op, _, _) in enumerate(us[name]) if op in (OP_ASSEMBLE, OP_IM2COL)] for name in us}
    assert len(uni_asm["step_active"]) == 2 and len(uni_asm["step_inactive"]) == 1 and not uni_asm["prologue"]
    for key, last_op in (("euler", OP_STEP), ("euler_custom", OP_STEP), ("eulera", OP_STEP_NOISE), ("heun", OP_STEP)):
        steps = 2 * n - 1 if key == "heun" else n
        bufs, segs = plan_dump(compiled[key])
        assert struct.unpack("<I", open(compiled[key], "rb").read()[4:8])[0] == 6           # a file with a version-6 op says so
        assert len(compiled["seq"][key]) == steps
        # pipe:1006-1012 over len(timesteps): the window [0, 0.67] of `steps` evaluations
        assert compiled["seq"][key] == ["step_active" if (i + 1) / steps <= 0.67 else "step_inactive" for i in range(steps)]
        for name in ("step_active", "step_inactive"):
            ops = [op for op, _, _ in segs[name]]
            assert OP_ASSEMBLE not in ops and OP_IM2COL not in ops, (key, name)
            # the launch list of the UniPC plan with every assembly swapped for its scaled form (and the step op, for the ancestral)
            want = [{OP_ASSEMBLE: OP_ASSEMBLE_SCALED, OP_IM2COL: OP_IM2COL_SCALED}.get(op, op) for op, _, _ in us[name]]
            assert ops[:-1] == want[:-1] and ops[-1] == last_op, (key, name)
            for i, uop in uni_asm[name]:
                op, sid, a = segs[name][i]
                ua = us[name][i][2]
                k = len(ua) - 1                                    # (coef, step_idx, nsteps) in front of the output
                assert len(a) == len(ua) + 3 and a[k + 2] == str(steps), (key, name, i)
                assert [_named(bufs, a[j]) for j in (k, k + 1)] == [("coef", 0), ("step_idx", 0)]
                # everything else is the unscaled launch's argument list: same named buffers, same integers, same output
                spell = lambda b_, args: [x if not x.startswith("p") or x == "p-" else _named(b_, x) for x in args]
                assert _named(bufs, a[0]) == ("latents", 0) and spell(bufs, a[:k] + a[-1:]) == spell(ub, ua), (key, name, i)
        assert ("variance_noise" in {nm for nm, _ in bufs.values()}) == (key == "eulera")
        # the stored tables are the scheduler's (guidance in column 11, the divisor in column 14, fractional timesteps unrounded)
        s, kw = compiled["scheds"][key]
        s.set_timesteps(timesteps=kw["timesteps"]) if "timesteps" in kw else s.set_timesteps(n)
        d = _stored(compiled[key])
        coef = np.frombuffer(d["coef"], np.float32).reshape(steps, 16)
        ref = s.table_impl.table().numpy().copy()
        ref[:, 11] = 7.5
        assert np.array_equal(coef, ref) and (coef[:, 14] > 1).all(), key
        assert np.array_equal(np.frombuffer(d["t_table"], np.float32), s.timesteps.numpy().astype(np.float32)), key
    assert np.frombuffer(_stored(compiled["euler_custom"])["t_table"], np.float32)[1] == 850.5
    assert np.array_equal(np.frombuffer(_stored(compiled["eulera"])["variance_noise"], np.float32), compiled["noise"].numpy().reshape(-1))


def test_compiled_plans_of_the_existing_schedulers_hold_no_new_op(compiled, plan_dump):
    ub, us = plan_dump(compiled["uni"])
    for key in ("uni", "ddim", "ddim_eta", "dpm", "dpm3", "sde"):
        assert struct.unpack("<I", open(compiled[key], "rb").read()[4:8])[0] == 5           # and stays a version-5 file
        bufs, segs = plan_dump(compiled[key])
        for name, recs in segs.items():
            ops = [op for op, _, _ in recs]
            assert OP_ASSEMBLE_SCALED not in ops and OP_IM2COL_SCALED not in ops and max(ops) < OP_ASSEMBLE_SCALED, (key, name)
            assert [op for op in ops if op in (OP_ASSEMBLE, OP_IM2COL)] == [op for op, _, _ in us[name] if op in (OP_ASSEMBLE, OP_IM2COL)]
        assert (np.frombuffer(_stored(compiled[key])["coef"], np.float32).reshape(-1, 16)[:, 14] == 0).all()
    st = compiled["stats"]
    # UniPC, DDIM and DPM-Solver++ 2M share one plan as before; a scaled plan is never theirs, nor the other way round
    assert st["ddim"]["plans_recorded"] == st["uni"]["plans_recorded"] and st["dpm"]["plans_recorded"] == st["ddim_eta"]["plans_recorded"]
    assert st["euler"]["plans_recorded"] == st["sde"]["plans_recorded"] + 1
    assert st["euler_custom"]["plans_recorded"] == st["euler"]["plans_recorded"]             # Euler on other timesteps: the same plan
    assert st["eulera"]["plans_recorded"] == st["euler"]["plans_recorded"] + 1 and st["heun"]["plans_recorded"] == st["eulera"]["plans_recorded"] + 1


def test_engine_refusals_for_the_new_kinds(tmp_path):
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from tests.gpu_common import tiny_trunk_configs
    usd, bsd = tiny_weights()
    ucfg, bcfg = tiny_trunk_configs()
    eng = BlobCtrlEngine(usd, bsd, ucfg, bcfg, device="cpu", scheduler="unipc", compile_only=True)
    path = str(tmp_path / "unused.bcplan")
    for cls in ("euler", "euler_ancestral", "heun"):
        s = _scheduler(cls)
        eng.set_scheduler(s.kind, s.table_params())
        with pytest.raises(NotImplementedError, match="eta"):
            eng.compile_plan(path, 1, 8, 8, 7, TINY["ctx"], 5, eta=0.5)
        if cls != "euler":
            with pytest.raises(NotImplementedError, match="timesteps"):
                eng.compile_plan(path, 1, 8, 8, 7, TINY["ctx"], 5, timesteps=[999, 500, 10])
        if cls != "euler_ancestral":
            with pytest.raises(ValueError):
                eng.compile_plan(path, 1, 8, 8, 7, TINY["ctx"], 5, variance_noise=torch.zeros(5, 1, 4, 8, 8))
    assert not os.path.exists(path)


def test_a_version_5_file_cannot_smuggle_a_version_6_op(compiled, plan_dump, tmp_path):
    """The parser accepts the scaled assemblies only in a file that says version 6; the version-6 file itself loads."""
    raw = bytearray(open(compiled["euler"], "rb").read())
    plan_dump(compiled["euler"])
    raw[4:8] = struct.pack("<I", 5)
    bad = tmp_path / "v5.bcplan"
    bad.write_bytes(bytes(raw))
    with pytest.raises(AssertionError, match="unknown op"):
        plan_dump(str(bad))
