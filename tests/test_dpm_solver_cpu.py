"""DPM-Solver++ without a GPU: the coefficient tables and the drop-in DPMSolverMultistepScheduler against the reference's
DPMSolverMultistepScheduler (tests/golden/schedulers_dpm.npz, dpm_config.json), the noise the reference drew (loop_tiny_dpm.npz,
pipeline_call_dpm.npz), and what compiled DPM plans launch (read back through the host-side `.bcplan` parser)."""
import json
import os

import numpy as np
import pytest
import torch

from tests.common import TINY, build_plan_dump, g, plan_named as _named, plan_stored as _stored, tiny_weights

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
OP_STEP, OP_STEP_NOISE, OP_STEP3 = 11, 30, 31
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000, steps_offset=1)


def _gold(name):
    return np.load(os.path.join(GOLD, name))


def _cases():
    z = _gold("schedulers_dpm.npz")
    return sorted(k[:-3] for k in z.files if k.endswith("_kw"))


def _case_kw(z, name):
    kw = json.loads(str(z[f"{name}_kw"]))
    return kw.pop("n"), kw.pop("timesteps"), kw


def _check_traj(got, ref, what):
    assert got.shape == ref.shape, what
    for i in range(1, ref.shape[0]):                         # the bar of test_host_cpu.py:98, per step
        err = np.abs(got[i] - ref[i]).max()
        assert err <= 5e-6 * np.abs(ref[i]).max(), (what, i, err)


@pytest.mark.parametrize("name", _cases())
def test_table_rows_reproduce_the_reference_trajectories(name):
    from blobctrl_amd.schedulers import DPMSolverMultistepTable, apply_table_step
    z = _gold("schedulers_dpm.npz")
    n, ts, kw = _case_kw(z, name)
    tab = DPMSolverMultistepTable(**{k: v for k, v in dict(SD, **kw).items() if k not in ("beta_schedule",)})
    tab.set_timesteps(timesteps=ts) if ts is not None else tab.set_timesteps(n)
    assert tab.timesteps.dtype == torch.int64 and np.array_equal(tab.timesteps.numpy(), z[f"{name}_timesteps"])
    assert np.array_equal(tab.sigmas.numpy(), z[f"{name}_sigmas"])
    assert torch.isfinite(tab.coef).all() and tab.coef.shape == (len(tab.timesteps), 16)
    assert (tab.coef[:, 11] == 0).all() and (tab.coef[:, 2:7] == 0).all() and (tab.coef[:, 10] == 0).all()
    assert bool((tab.coef[:, 12] != 0).any()) == tab.sde
    assert bool((tab.coef[:, 13] != 0).any()) == (3 in tab.step_orders())
    ref = z[f"{name}_traj"]
    x = torch.from_numpy(ref[0])
    zz = torch.zeros_like(x)
    hist = dict(m0=zz, m1=zz.clone(), last=zz.clone())
    xs = [x]
    for i in range(len(tab.timesteps)):
        noise = g(200 + i, 1, 4, 8, 8) if tab.sde else None
        x = apply_table_step(tab.coef[i].tolist(), g(100 + i, 1, 4, 8, 8), x, hist, noise)
        xs.append(x)
    _check_traj(torch.stack(xs).numpy(), ref, name)


def test_orders_and_the_final_zero_sigma_row():
    from blobctrl_amd.schedulers import DPMSolverMultistepTable
    o = lambda n, **kw: DPMSolverMultistepTable(**kw).set_timesteps(n).step_orders()
    assert o(14) == [1] + [2] * 11 + [2, 1]
    assert o(15) == [1] + [2] * 13 + [1]                          # 15 steps: lower_order_final only through the zero final sigma
    assert o(15, final_sigmas_type="sigma_min") == [1] + [2] * 14
    assert o(15, final_sigmas_type="sigma_min", euler_at_final=True) == [1] + [2] * 13 + [1]
    assert o(6, solver_order=3) == [1, 2, 3, 3, 2, 1]
    assert o(5, solver_order=1) == [1] * 5
    for sde in ("dpmsolver++", "sde-dpmsolver++"):
        tab = DPMSolverMultistepTable(algorithm_type=sde).set_timesteps(20)
        last = tab.coef[-1]
        assert tab.sigmas[-1] == 0 and last[7] == 0 and last[12] == 0 and last[9] == 0
        assert torch.allclose(last[8], torch.tensor(1.0)) and torch.isfinite(tab.coef).all()


def test_existing_rows_have_no_column_13():
    from blobctrl_amd.schedulers import DDIMTable, UniPCTable, apply_table_step
    for tab in (UniPCTable().set_timesteps(20), DDIMTable().set_timesteps(20), DDIMTable().set_timesteps(20, eta=1.0)):
        assert (tab.coef[:, 13] == 0).all()
    # a non-zero column 13 adds c13 * x0_{i-2}, and nothing else
    row = [0.0] * 16
    row[13] = 0.25
    hist = dict(m0=torch.zeros(3), m1=torch.full((3,), 4.0), last=torch.zeros(3))
    assert torch.equal(apply_table_step(row, torch.zeros(3), torch.zeros(3), hist), torch.full((3,), 1.0))


def test_dropin_config_matches_the_reference():
    from blobctrl_amd.schedulers import DPMSolverMultistepScheduler, PNDMScheduler
    ref = json.load(open(os.path.join(GOLD, "dpm_config.json")))
    s = DPMSolverMultistepScheduler.from_config(ref["source"])
    cfg = dict(s.config)
    cfg["_use_default_values"] = sorted(cfg["_use_default_values"])
    assert cfg == ref["config"]
    # through the PNDM configuration holder the scripts start from: the same values for every DPM-Solver key
    p = PNDMScheduler(**{k: v for k, v in ref["source"].items() if not k.startswith("_") and k != "trained_betas"})
    s2 = DPMSolverMultistepScheduler.from_config(p.config)
    for k in set(DPMSolverMultistepScheduler._defaults) | {"beta_start", "beta_end", "num_train_timesteps", "steps_offset"}:
        assert s2.config[k] == ref["config"][k], k
    assert s2.config.timestep_spacing == "linspace" and s2.config.steps_offset == 1
    s2.set_timesteps(20)
    assert s2.timesteps[:3].tolist() == [999, 949, 899] and s2.order == 1 and s2.init_noise_sigma == 1.0
    import copy
    copy.deepcopy(s2)
    # option overrides through from_config (what "DPM++ 2M Karras" is)
    k = DPMSolverMultistepScheduler.from_config(p.config, use_karras_sigmas=True)
    assert k.config.use_karras_sigmas and "use_karras_sigmas" not in k.config._use_default_values
    assert k.table_params()[:3] == (1000, 0.00085, 0.012) and ("use_karras_sigmas", True) in k.table_params()[3]


def test_set_timesteps_errors_and_refused_options():
    from blobctrl_amd.schedulers import DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler()
    with pytest.raises(ValueError, match="exactly one"):
        s.set_timesteps()
    with pytest.raises(ValueError, match="Can only pass one"):
        s.set_timesteps(10, timesteps=[999, 500])
    with pytest.raises(ValueError, match="use_karras_sigmas"):
        DPMSolverMultistepScheduler(use_karras_sigmas=True).set_timesteps(timesteps=[999, 500])
    with pytest.raises(ValueError, match="use_lu_lambdas"):
        DPMSolverMultistepScheduler(use_lu_lambdas=True).set_timesteps(timesteps=[999, 500])
    with pytest.raises(ValueError, match="final_sigmas_type"):
        DPMSolverMultistepScheduler(final_sigmas_type="nope").set_timesteps(10)
    with pytest.raises(ValueError, match="Number of inference steps"):
        DPMSolverMultistepScheduler().step(torch.zeros(1, 4, 8, 8), 999, torch.zeros(1, 4, 8, 8))
    for kw, word in ((dict(algorithm_type="dpmsolver"), "algorithm_type"), (dict(algorithm_type="sde-dpmsolver"), "algorithm_type"),
                     (dict(thresholding=True), "thresholding"), (dict(variance_type="learned"), "variance_type"),
                     (dict(variance_type="learned_range"), "variance_type"),
                     (dict(algorithm_type="sde-dpmsolver++", solver_order=3), "solver_order=3")):
        with pytest.raises(NotImplementedError, match=word):
            DPMSolverMultistepScheduler(**kw)
    assert DPMSolverMultistepScheduler(solver_type="bh2").config.solver_type == "midpoint"     # re-registered like the reference


def test_dropin_step_reproduces_the_reference_including_sde_noise():
    from blobctrl_amd.schedulers import DPMSolverMultistepScheduler
    z = _gold("schedulers_dpm.npz")

    def run(s, kw_of_step, n=None, ts=None):
        s.set_timesteps(n, timesteps=ts)
        x = g(21, 1, 4, 8, 8)
        xs = [x]
        for i, t in enumerate(s.timesteps):
            out = s.step(g(100 + i, 1, 4, 8, 8), t, x, **kw_of_step(i))
            x = out[0] if isinstance(out, tuple) else out.prev_sample
            xs.append(x)
        return torch.stack(xs).numpy()

    for name in ("pp2_mid_karras_50", "pp3_custom_10", "sde2_mid_lin_15", "sde2_custom_10", "sde1_lin_5"):
        n, ts, kw = _case_kw(z, name)
        s = DPMSolverMultistepScheduler(**dict(SD, **kw))
        got = run(s, lambda i: dict(variance_noise=g(200 + i, 1, 4, 8, 8), return_dict=(i % 2 == 0)), n, ts)
        _check_traj(got, z[f"{name}_traj"], name)
    s = DPMSolverMultistepScheduler(**SD, algorithm_type="sde-dpmsolver++")
    gen = torch.Generator().manual_seed(77)
    _check_traj(run(s, lambda i: dict(generator=gen), 5), z["sde2_gen77_5_traj"], "generator")
    # deterministic DPM-Solver++ ignores generator and variance_noise, as the reference does
    s = DPMSolverMultistepScheduler(**SD)
    a = run(s, lambda i: dict(), 5)
    b = run(s, lambda i: dict(generator=torch.Generator().manual_seed(1), variance_noise=g(9, 1, 4, 8, 8)), 5)
    assert np.array_equal(a, b)


def test_noise_helper_draws_what_the_reference_drew():
    from blobctrl_amd.pipeline import BlobCtrlEngine
    z = _gold("loop_tiny_dpm.npz")
    ref = z["sde2m_5_noise"]
    got = BlobCtrlEngine.variance_noise(ref.shape[0], 1, 8, 8, torch.Generator().manual_seed(int(z["sde2m_5_seed"])), device="cpu")
    assert np.array_equal(got.numpy(), ref)
    # __call__: the generator draws the start latents first, then every step's noise
    zc = _gold("pipeline_call_dpm.npz")
    gen = torch.Generator().manual_seed(int(zc["seed"]))
    B = zc["latents"].shape[0]
    torch.randn((B, 4, 8, 8), generator=gen, dtype=torch.float32)
    got = BlobCtrlEngine.variance_noise(len(zc["timesteps"]), B, 8, 8, gen, device="cpu")
    assert np.array_equal(got.numpy(), zc["noise"])


def test_scheduler_config_dir_and_engine_tables():
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from blobctrl_amd.schedulers import DPMSolverMultistepScheduler, DPMSolverMultistepTable, UniPCMultistepScheduler
    eng = BlobCtrlEngine.__new__(BlobCtrlEngine)
    eng._sched_cache, eng.scheduler_kind, eng.scheduler_params = {}, "unipc", (1000, 0.00085, 0.012)
    s = DPMSolverMultistepScheduler(use_karras_sigmas=True, solver_order=3)
    eng.set_scheduler(s.kind, s.table_params())
    tab = eng._scheduler_table(20)
    s.set_timesteps(20)
    assert torch.equal(tab.table(), s.table_impl.table()) and torch.equal(tab.timesteps, s.timesteps)
    assert eng._step_form(tab, False) == (False, True)
    ts = [999, 850, 736, 645, 545, 455, 343, 233, 124, 24]
    eng.set_scheduler("dpmsolver", DPMSolverMultistepScheduler().table_params())
    t2 = eng._scheduler_table(len(ts), timesteps=ts)
    assert t2.timesteps.tolist() == ts and eng._step_form(t2, False) == (False, False)
    assert torch.equal(t2.table(), DPMSolverMultistepTable().set_timesteps(timesteps=ts).table())
    eng.set_scheduler("dpmsolver", DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++").table_params())
    assert eng._step_form(eng._scheduler_table(10), False) == (True, False)
    u = UniPCMultistepScheduler()
    eng.set_scheduler(u.kind, u.table_params())
    with pytest.raises(NotImplementedError, match="timesteps"):
        eng._scheduler_table(10, timesteps=ts)


# ------------------------------------------------------------------------------------------------------------ compiled plans
@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    return build_plan_dump(tmp_path_factory.mktemp("dump"))


def test_compiled_dpm_plans(plan_dump, tmp_path):
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from blobctrl_amd.schedulers import DPMSolverMultistepScheduler, DPMSolverMultistepTable, UniPCMultistepScheduler
    from tests.gpu_common import tiny_trunk_configs
    usd, bsd = tiny_weights()
    ucfg, bcfg = tiny_trunk_configs()
    eng = BlobCtrlEngine(usd, bsd, ucfg, bcfg, device="cpu", scheduler="unipc", compile_only=True)
    n, B, h, w, T = 6, 1, 8, 8, 7
    paths = {k: str(tmp_path / f"{k}.bcplan") for k in ("uni", "dpm2", "sde", "dpm3", "custom")}

    def use(s):
        eng.set_scheduler(s.kind, s.table_params())

    use(UniPCMultistepScheduler())
    eng.compile_plan(paths["uni"], B, h, w, T, TINY["ctx"], n)
    recorded = eng.cache_stats["plans_recorded"]
    use(DPMSolverMultistepScheduler(use_karras_sigmas=True))
    eng.compile_plan(paths["dpm2"], B, h, w, T, TINY["ctx"], n)
    assert eng.cache_stats["plans_recorded"] == recorded                      # UniPC -> DPM++ 2M: the same plan, other tables
    noise = g(5, n, B, 4, h, w)
    use(DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++"))
    eng.compile_plan(paths["sde"], B, h, w, T, TINY["ctx"], n, variance_noise=noise)
    use(DPMSolverMultistepScheduler(solver_order=3))
    eng.compile_plan(paths["dpm3"], B, h, w, T, TINY["ctx"], n)
    ts = [999, 850, 736, 645, 545, 455, 343, 233, 124, 24]
    use(DPMSolverMultistepScheduler())
    assert eng.compile_plan(paths["custom"], B, h, w, T, TINY["ctx"], 50, timesteps=ts) == ["step_active"] * len(ts)
    with pytest.raises(NotImplementedError, match="eta"):
        eng.compile_plan(paths["custom"], B, h, w, T, TINY["ctx"], n, eta=0.5)

    ub, us = plan_dump(paths["uni"])
    for key, last_op, nargs in (("dpm2", OP_STEP, 11), ("sde", OP_STEP_NOISE, 13), ("dpm3", OP_STEP3, 12), ("custom", OP_STEP, 11)):
        bufs, segs = plan_dump(paths[key])
        assert ("variance_noise" in {nm for nm, _ in bufs.values()}) == (key == "sde"), key
        for name in ("step_active", "step_inactive"):
            ops = [op for op, _, _ in segs[name]]
            # per-step cost unchanged by construction: the launch list of the UniPC plan, the step op swapped at most
            assert ops[:-1] == [op for op, _, _ in us[name]][:-1] and ops[-1] == last_op, (key, name)
            assert [op for op in ops if op in (OP_STEP, OP_STEP_NOISE, OP_STEP3)] == [last_op]
            a = segs[name][-1][2]
            assert len(a) == nargs and a[5:9] == ["-1", "1", "8", "8"]
            assert [_named(bufs, a[k]) for k in (1, 2, 3, 4)] == [("latents", 0), ("coef", 0), ("step_idx", 0), ("hist", 0)]
            if key == "dpm3":                                                  # "pppppfiiiipi": nsteps, eps_out, advance
                assert a[9] == str(n) and _named(bufs, a[10]) == ("eps_guided", 0) and a[11] == "1"
            if key == "sde":
                assert _named(bufs, a[9]) == ("variance_noise", 0) and a[10] == str(n)
    # the stored coefficient table is the scheduler's table (guidance in column 11)
    for key, s, steps, kw in (("dpm2", DPMSolverMultistepScheduler(use_karras_sigmas=True), n, {}),
                              ("sde", DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++"), n, {}),
                              ("dpm3", DPMSolverMultistepScheduler(solver_order=3), n, {}),
                              ("custom", DPMSolverMultistepScheduler(), len(ts), dict(timesteps=ts))):
        d = _stored(paths[key])
        coef = np.frombuffer(d["coef"], np.float32).reshape(steps, 16)
        s.set_timesteps(None if kw else steps, **kw)
        ref = s.table_impl.table().numpy().copy()
        ref[:, 11] = 7.5
        assert np.array_equal(coef, ref), key
        assert np.array_equal(np.frombuffer(d["t_table"], np.float32), s.timesteps.numpy().astype(np.float32)), key
    assert np.array_equal(np.frombuffer(_stored(paths["sde"])["variance_noise"], np.float32), noise.numpy().reshape(-1))
    assert (np.frombuffer(_stored(paths["dpm3"])["coef"], np.float32).reshape(n, 16)[:, 13] != 0).any()
    assert DPMSolverMultistepTable(solver_order=3).set_timesteps(n).step_orders() == [1, 2, 3, 3, 2, 1]


def test_pipeline_refuses_custom_timesteps_without_dpm_solver_and_eta_with_it():
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from blobctrl_amd.schedulers import DPMSolverMultistepScheduler
    from tests.gpu_common import tiny_trunk_configs
    usd, bsd = tiny_weights()
    ucfg, bcfg = tiny_trunk_configs()
    eng = BlobCtrlEngine(usd, bsd, ucfg, bcfg, device="cpu", scheduler="ddim", compile_only=True)
    path = "unused.bcplan"
    with pytest.raises(NotImplementedError, match="timesteps"):
        eng.compile_plan(path, 1, 8, 8, 7, TINY["ctx"], 5, timesteps=[999, 500, 10])
    s = DPMSolverMultistepScheduler()
    eng.set_scheduler(s.kind, s.table_params())
    with pytest.raises(NotImplementedError, match="DDIM"):
        eng.compile_plan(path, 1, 8, 8, 7, TINY["ctx"], 5, eta=1.0)
    with pytest.raises(ValueError):
        eng.compile_plan(path, 1, 8, 8, 7, TINY["ctx"], 5, variance_noise=torch.zeros(5, 1, 4, 8, 8))
    assert not os.path.exists(path)
