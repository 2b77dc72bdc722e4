"""Request batches whose requests run their own schedules, host side: the stacked per-request tables (`schedulers.request_tables`: a
request's rows are its own table's bit for bit, finished rows behind them), the host trajectory of two requests of different lengths at
once against the scheduler fixtures, every refusal of a call with lists (before a plan is recorded), what a compiled mixed plan holds
(a version-8 file whose step segments end in bc_scheduler_step_requests), the dispatcher op, and that scalar plans compile to the listing
they had (plan_listings_before_requests.json: written by the commit before per-request schedules) and store the tables they stored
(plan_tables_before_setup_merge.json: written by the commit before `denoise` / `compile_plan` got one shared set-up)."""
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
OP_STEP_REQUESTS, OP_ASM_REQUESTS, OP_IM2COL_REQUESTS, OP_TEMB_ROWS = 38, 39, 40, 41
STEPS, GUIDANCE = (4, 6, 5), (7.5, 3.0, 1.0)


def _gold(name):
    return np.load(os.path.join(GOLD, name))


def _factories():
    """name -> (table factory, per-request eta or None): every scheduler kind of the engine, DPM-Solver++ in its three step forms."""
    from blobctrl_amd.schedulers import (DDIMTable, DPMSolverMultistepTable, EulerAncestralTable, EulerDiscreteTable, HeunTable, LCMTable,
                                         UniPCTable)
    return {"unipc": (UniPCTable, None), "ddim": (DDIMTable, None), "ddim_eta": (DDIMTable, [0.0, 0.5, 1.0]),
            "dpm_2m_karras": (lambda: DPMSolverMultistepTable(use_karras_sigmas=True), None),
            "dpm_3m": (lambda: DPMSolverMultistepTable(solver_order=3), None),
            "dpm_sde": (lambda: DPMSolverMultistepTable(algorithm_type="sde-dpmsolver++"), None),
            "euler": (EulerDiscreteTable, None), "euler_ancestral": (EulerAncestralTable, None), "heun": (HeunTable, None),
            "lcm": (LCMTable, None)}


# ------------------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("name", sorted(_factories()))
def test_a_requests_rows_are_its_own_tables_rows(name):
    from blobctrl_amd.schedulers import request_tables
    factory, eta = _factories()[name]
    coef, t_rows, evals = request_tables(factory, list(STEPS), list(GUIDANCE), eta)
    nmax = max(evals)
    assert coef.shape == (3, nmax, 16) and coef.dtype == torch.float32 and t_rows.shape == (nmax, 3) and t_rows.dtype == torch.float32
    for b, n in enumerate(STEPS):
        own = factory()
        own.set_timesteps(n, eta=eta[b]) if eta is not None else own.set_timesteps(n)
        e = own.coef.shape[0]
        assert evals[b] == e == (2 * n - 1 if name == "heun" else n)
        cols = [c for c in range(16) if c != 11]
        assert torch.equal(coef[b, :e][:, cols], own.coef[:, cols]), (name, b)          # bit for bit, the guidance column apart
        assert (own.coef[:, 11] == 0).all() and (own.coef[:, 15] == 0).all()             # (both free in every scheduler's own table)
        assert torch.equal(t_rows[:e, b], own.timesteps.to(torch.float32)), (name, b)
        # finished rows: the flag, "do not divide", nothing else but the request's guidance scale; the last timestep repeated
        assert (coef[b, :e, 15] == 0).all() and (coef[b, e:, 15] == 1).all() and (coef[b, e:, 14] == 1).all()
        assert (coef[b, e:][:, [c for c in range(16) if c not in (11, 14, 15)]] == 0).all()
        assert (coef[b, :, 11] == np.float32(GUIDANCE[b])).all()
        assert (t_rows[e:, b] == t_rows[e - 1, b]).all()
    if eta is not None:                                                                  # per-request eta: the noise coefficient
        assert (coef[0, :, 12] == 0).all() and (coef[1, :6, 12] > 0).all() and (coef[2, :5, 12] > coef[1, :5, 12].min()).all()


def test_request_tables_takes_timestep_lists_and_refuses_a_wrong_count():
    from blobctrl_amd.schedulers import DDIMTable, DPMSolverMultistepTable, request_tables
    ts = [[999, 500, 10], [901, 601, 301, 1]]
    coef, t_rows, evals = request_tables(DPMSolverMultistepTable, ts, [2.0, 3.0])
    assert evals == [3, 4] and t_rows[:, 0].tolist() == [999, 500, 10, 10] and t_rows[:, 1].tolist() == [901, 601, 301, 1]
    own = DPMSolverMultistepTable().set_timesteps(timesteps=ts[0])
    assert torch.equal(coef[0, :3, :11], own.coef[:, :11])
    with pytest.raises(ValueError, match="eta"):
        request_tables(DDIMTable, [3, 4], [1.0, 1.0], eta=[0.5])
    with pytest.raises(ValueError, match="guidance"):
        request_tables(DDIMTable, [3, 4], [1.0])


# ------------------------------------------------------------------------------------------------------------ host trajectory
def _check_traj(got, ref, what):
    assert got.shape == ref.shape, what
    for i in range(1, ref.shape[0]):                         # the bar of test_host_cpu.py:98, per step
        err = np.abs(got[i] - ref[i]).max()
        assert err <= 5e-6 * np.abs(ref[i]).max(), (what, i, err)


def _drive(coef, evals, starts, noisy):
    """Both requests through `apply_table_step`, step by step from the stacked table, a finished request left alone: the trajectories."""
    from blobctrl_amd.schedulers import apply_table_step
    B, nmax = coef.shape[0], coef.shape[1]
    x = [s.clone() for s in starts]
    hist = [dict(m0=torch.zeros_like(s), m1=torch.zeros_like(s), last=torch.zeros_like(s)) for s in starts]
    traj = [[s.clone()] for s in starts]
    for i in range(nmax):
        for b in range(B):
            row = coef[b, i].tolist()
            assert (row[15] != 0) == (i >= evals[b])
            if row[15] != 0:
                continue
            x[b] = apply_table_step(row, g(100 + i, 1, 4, 8, 8), x[b], hist[b], g(200 + i, 1, 4, 8, 8) if noisy else None)
            traj[b].append(x[b])
    return [torch.stack(t).numpy() for t in traj]


@pytest.mark.parametrize("fixture, a, b", [("schedulers.npz", "unipc_5", "unipc_20"), ("schedulers.npz", "ddim_20", "ddim_5"),
                                           ("schedulers_dpm.npz", "pp2_mid_lin_5", "pp2_mid_lin_14"),
                                           ("schedulers_dpm.npz", "pp3_lin_14", "pp3_lin_5"),
                                           ("schedulers_dpm.npz", "pp2_mid_karras_50", 7), ("schedulers_dpm.npz", "sde2_mid_lin_15", 5),
                                           ("schedulers_euler.npz", "euler_leading_5", "euler_leading_20"),
                                           ("schedulers_euler.npz", "eulera_noise_15", 4), ("schedulers_euler.npz", "heun_10", 3)])
def test_two_requests_of_different_lengths_follow_the_reference_trajectories(fixture, a, b):
    """One scheduler configuration, two step counts at once: each request, driven from the stacked table, lands on the reference
    trajectory of its own step count, and is bit for bit the request driven alone from its own table.  (`b` an int: the fixture holds
    no second case of that configuration - the second request is then checked against its run alone only.)"""
    from blobctrl_amd.schedulers import request_tables, table_class
    z = _gold(fixture)
    if fixture == "schedulers.npz":
        kind, opts = a.split("_")[0], {}
    else:
        kw = json.loads(str(z[f"{a}_kw"]))
        kind = kw.pop("cls", "dpmsolver")
        kw.pop("n"), kw.pop("timesteps")
        Table = table_class(kind)
        opts = {k: v for k, v in dict(SD, **kw).items() if k != "beta_schedule" and
                (kind == "dpmsolver" or k != "steps_offset" or k in Table._option_defaults)}
    factory = lambda: table_class(kind)(**opts)
    steps = [int(a.rsplit("_", 1)[1]), b if isinstance(b, int) else int(b.rsplit("_", 1)[1])]
    coef, t_rows, evals = request_tables(factory, steps, [7.5, 2.0])
    tables = [factory().set_timesteps(n) for n in steps]
    noisy = bool(getattr(tables[0], "sde", False))
    starts = [torch.from_numpy(z[f"{a}_traj"][0]),
              g(21, 1, 4, 8, 8) * tables[1].init_noise_sigma if isinstance(b, int) else torch.from_numpy(z[f"{b}_traj"][0])]
    got = _drive(coef, evals, starts, noisy)
    assert [len(t) - 1 for t in got] == evals and evals[0] != evals[1]
    _check_traj(got[0], z[f"{a}_traj"], a)
    if not isinstance(b, int):
        _check_traj(got[1], z[f"{b}_traj"], b)
    for k in range(2):
        assert np.array_equal(got[k], _drive(tables[k].coef[None], [evals[k]], [starts[k]], noisy)[0])


# ------------------------------------------------------------------------------------------------------------ refusals
def _engine(scheduler="unipc"):
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from tests.gpu_common import tiny_trunk_configs
    usd, bsd = tiny_weights()
    ucfg, bcfg = tiny_trunk_configs()
    return BlobCtrlEngine(usd, bsd, ucfg, bcfg, device="cpu", scheduler=scheduler, compile_only=True, max_cached_plans=16)


def _batch(B=3):
    return dict(prompt_embeds=g(1, 2 * B, 7, TINY["ctx"]), fg_image_latents=g(2, B, 4, 8, 8), bg_image_latents=g(3, B, 4, 8, 8),
                gs_score=g(4, B, 2, 8, 8).abs(), dino_feats=g(5, B, 1, TINY["feat"]), latents=g(6, B, 4, 8, 8))


def test_every_refusal_is_raised_before_a_plan_is_recorded(tmp_path):
    from blobctrl_amd.schedulers import (DDIMScheduler, EulerAncestralDiscreteScheduler, HeunDiscreteScheduler, LCMScheduler,
                                         UniPCMultistepScheduler)
    eng = _engine()
    three, one = _batch(3), _batch(1)
    ts3 = [[999, 500, 10], [900, 400], [800, 300, 100, 1]]
    for call in (eng.denoise, eng):                                              # (`__call__` hands what it cannot route to `denoise`)
        # a list without a request batch, or of the wrong length: the keyword and B
        for kw, name in ((dict(num_inference_steps=[4]), "num_inference_steps"), (dict(guidance_scale=[7.5]), "guidance_scale"),
                         (dict(blobnet_control_guidance_start=[0.0]), "blobnet_control_guidance_start"),
                         (dict(blobnet_control_guidance_end=[1.0]), "blobnet_control_guidance_end")):
            with pytest.raises(ValueError, match=rf"{name}.*request batch.*B = 1"):
                call(**one, **kw)
            with pytest.raises(ValueError, match=rf"{name}: expected 3 values \(one per request, B = 3\), got 1"):
                call(**three, **kw)
        # entry types
        for kw in (dict(guidance_scale=[7.5, 3, 1.0]), dict(blobnet_control_guidance_start=[0, 0.0, 0.0]),
                   dict(blobnet_control_guidance_end=[1.0, 1, 1.0]), dict(num_inference_steps=[4, 5.0, 6]),
                   dict(num_inference_steps=[4, 5, 6], blobnet_conditioning_scale=[1.0, 1, 1.0])):
            with pytest.raises(TypeError, match="must be"):
                call(**three, **kw)
        # windows: today's message with the request index
        with pytest.raises(ValueError, match=r"request 1: control guidance start: 0.5 cannot be larger or equal to control guidance end: 0.5"):
            call(**three, blobnet_control_guidance_start=[0.0, 0.5, 0.0], blobnet_control_guidance_end=[1.0, 0.5, 1.0])
        with pytest.raises(ValueError, match=r"request 2: control guidance start: -0.1 can't be smaller than 0"):
            call(**three, blobnet_control_guidance_start=[0.0, 0.0, -0.1])
        with pytest.raises(ValueError, match=r"request 0: control guidance end: 1.5 can't be larger than 1.0"):
            call(**three, blobnet_control_guidance_end=[1.5, 1.0, 1.0])
        with pytest.raises(ValueError, match=r"request 1: num_inference_steps must be >= 1"):
            call(**three, num_inference_steps=[4, 0, 4])
    with pytest.raises(ValueError, match=r"eta: expected 3 values"):
        eng.denoise(**three, eta=[0.0, 0.5])
    with pytest.raises(NotImplementedError, match="eta != 0 is supported with DDIM only"):        # eta: DDIM only, as today
        eng.denoise(**three, eta=[0.0, 0.5, 1.0])
    with pytest.raises(ValueError, match=r"timesteps: expected 3 values"):
        eng.denoise(**three, timesteps=ts3[:2])
    # per-request timesteps: refused exactly as the scalar ones are
    for s in (UniPCMultistepScheduler(), DDIMScheduler(), HeunDiscreteScheduler(**SD), EulerAncestralDiscreteScheduler(**SD)):
        eng.set_scheduler(s.kind, s.table_params())
        with pytest.raises(NotImplementedError) as scalar:
            eng.denoise(**one, timesteps=ts3[0])
        with pytest.raises(NotImplementedError) as listed:
            eng.denoise(**three, timesteps=ts3)
        assert str(listed.value) == str(scalar.value) and "custom `timesteps` are not tabulated" in str(listed.value)
        with pytest.raises(NotImplementedError, match="custom `timesteps` are not tabulated"):
            eng.compile_plan(str(tmp_path / "x.bcplan"), 3, 8, 8, 7, TINY["ctx"], None, timesteps=ts3)
    # the noise of a mixed edit has the loop's length; a third-order row and a noise row do not share a plan
    s = DDIMScheduler()
    eng.set_scheduler(s.kind, s.table_params())
    with pytest.raises(ValueError, match=r"variance_noise must have shape \(6, 3, 4, 8, 8\)"):
        eng.denoise(**three, num_inference_steps=[4, 6, 5], eta=[0.0, 0.5, 1.0], variance_noise=torch.zeros(5, 3, 4, 8, 8))
    with pytest.raises(ValueError, match="variance_noise is only used"):
        eng.denoise(**three, num_inference_steps=[4, 6, 5], variance_noise=torch.zeros(6, 3, 4, 8, 8))
    s = LCMScheduler()
    eng.set_scheduler(s.kind, s.table_params())
    with pytest.raises(ValueError, match="single_pass=True needs guidance off"):
        eng.denoise(**three, num_inference_steps=[2, 4, 3], guidance_scale=[1.0, 1.0, 2.0], single_pass=True)
    # compile_plan takes the same lists and refuses the same way
    eng.set_scheduler("unipc")
    with pytest.raises(ValueError, match=r"guidance_scale: expected 3 values"):
        eng.compile_plan(str(tmp_path / "x.bcplan"), 3, 8, 8, 7, TINY["ctx"], [4, 5, 6], guidance_scale=[7.5, 7.5])
    with pytest.raises(ValueError, match="request batch"):
        eng.compile_plan(str(tmp_path / "x.bcplan"), 1, 8, 8, 7, TINY["ctx"], [4])
    with pytest.raises(TypeError, match="list of `int`"):
        eng.compile_plan(str(tmp_path / "x.bcplan"), 3, 8, 8, 7, TINY["ctx"], [4, 5, "6"])
    with pytest.raises(ValueError, match="request 2: control guidance start"):
        eng.compile_plan(str(tmp_path / "x.bcplan"), 3, 8, 8, 7, TINY["ctx"], [4, 5, 6], blobnet_control_guidance_start=[0.0, 0.0, 1.0])
    with pytest.raises(ValueError, match="per-request schedules need a request batch"):
        eng.plan_for(3, 8, 8, 7, TINY["ctx"], 6, requests=True)
    assert eng.cache_stats["plans_recorded"] == 0 and not eng._plans and not os.path.exists(tmp_path / "x.bcplan")


# ------------------------------------------------------------------------------------------------------------ compiled plans
@pytest.fixture(scope="module")
def dump_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("dump")


@pytest.fixture(scope="module")
def plan_dump(dump_dir):
    return build_plan_dump(dump_dir)


def _version(path):
    return struct.unpack("<I", open(path, "rb").read()[4:8])[0]


MIXED = dict(guidance_scale=[7.5, 3.0, 1.0], blobnet_control_guidance_start=[0.0, 0.2, 0.0], blobnet_control_guidance_end=[1.0, 0.7, 0.5],
             blobnet_conditioning_scale=[1.0, 0.0, 1.7])


@pytest.mark.parametrize("kind", ["ddim", "euler", "dpm_sde", "dpm_3m", "lcm"])
def test_a_compiled_mixed_plan_is_a_version_8_file_that_ends_its_steps_in_the_requests_step(kind, plan_dump, tmp_path):
    from blobctrl_amd.pipeline import blobnet_keep
    from blobctrl_amd.schedulers import (DDIMScheduler, DPMSolverMultistepScheduler, EulerDiscreteScheduler, LCMScheduler,
                                         request_tables, table_class)
    s = {"ddim": DDIMScheduler(), "euler": EulerDiscreteScheduler(**SD), "dpm_sde": DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++"),
         "dpm_3m": DPMSolverMultistepScheduler(solver_order=3), "lcm": LCMScheduler()}[kind]
    eng = _engine()
    eng.set_scheduler(s.kind, s.table_params())
    B, h, w, T, D = 3, 8, 8, 7, TINY["ctx"]
    kw = dict(MIXED, guidance_scale=[1.0, 1.0, 0.5]) if kind == "lcm" else MIXED          # (LCM: guidance off, hence single-pass)
    path = str(tmp_path / "mixed.bcplan")
    seq = eng.compile_plan(path, B, h, w, T, D, list(STEPS), **kw)
    assert seq == ["step_active"] * 4 + ["step_inactive"] * 2                  # active while ANY request is: 0-3 of request 0, 0-1 of request 2
    key = next(reversed(eng._plans))
    assert key[-1] == "requests" and key[:7] == (B, h, w, T, D, 6, True) and eng.cache_stats["plans_recorded"] == 1
    assert _version(path) == 8
    single, noisy, third, scaled = kind == "lcm", kind in ("dpm_sde", "lcm"), kind == "dpm_3m", kind == "euler"
    Bu = B if single else 2 * B
    bufs, segs = plan_dump(path)
    sizes = {n_: b_ for n_, b_ in bufs.values() if n_ != "-"}
    assert sizes["coef"] == B * 6 * 16 * 4 and sizes["t_rows_unet"] == 6 * Bu * 4 and sizes["t_rows_blob"] == 6 * B * 4
    assert sizes["scale_table"] == 6 * B * 4 and "t_table" not in sizes and sizes["ctx"] == Bu * T * D * 2
    assert ("variance_noise" in sizes) == noisy and (not noisy or sizes["variance_noise"] == 6 * B * 4 * h * w * 4)
    for name in ("latents", "fg_lat", "bg_lat"):
        assert sizes[name] == B * 4 * h * w * 4
    for name in ("step_active", "step_inactive"):
        ops = [op for op, _, _ in segs[name]]
        op, sid, a = segs[name][-1]
        assert op == OP_STEP_REQUESTS and sid == 0 and ops.count(OP_STEP_REQUESTS) == 1
        assert not {11, 30, 31, 34} & set(ops)                                  # none of the scalar step forms
        assert [_named(bufs, a[j])[0] for j in (1, 2, 3, 4, 12)] == ["latents", "coef", "step_idx", "hist", "eps_guided"]
        assert a[5:8] == [str(B), str(h), str(w)] and a[9:12] == ["6", str(int(third)), str(int(single))] and a[13] == "1"
        assert (a[8] != "p-") == noisy and (not noisy or _named(bufs, a[8])[0] == "variance_noise")
        # assemblies: the per-image divisor forms exactly when the table scales its input
        asm = [(op_, a_) for op_, _, a_ in segs[name] if op_ in (8, 23, 32, 33, OP_ASM_REQUESTS, OP_IM2COL_REQUESTS)]
        assert len(asm) == (2 if name == "step_active" else 1)
        for op_, a_ in asm:
            assert (op_ in (OP_ASM_REQUESTS, OP_IM2COL_REQUESTS)) == scaled and op_ not in (32, 33)
            if scaled:
                assert [_named(bufs, a_[j])[0] for j in (9, 10)] == ["coef", "step_idx"] and a_[11] == "6"
    # the prologue tabulates the time embedding per step AND image, for both nets, and with no other embedding launch
    temb = sorted((a_[1], _named(bufs, a_[0])[0]) for op_, _, a_ in segs["prologue"] if op_ == OP_TEMB_ROWS)
    assert temb == sorted([(str(6 * Bu), "t_rows_unet"), (str(6 * B), "t_rows_blob")])
    assert not [op_ for op_, _, _ in segs["prologue"] if op_ in (9, 10, 35, 36)]
    # the stored tables are request_tables' and the windows' own
    Table = table_class(s.kind)
    opts = dict(s.table_params()[3]) if len(s.table_params()) > 3 else {}
    gs = [1.0, 1.0, 1.0] if kind == "lcm" else [7.5, 3.0, 1.0]
    coef, t_rows, evals = request_tables(lambda: Table(**opts), list(STEPS), gs)
    st = _stored(path)
    assert np.array_equal(np.frombuffer(st["coef"], np.float32).reshape(B, 6, 16), coef.numpy())
    assert np.array_equal(np.frombuffer(st["t_rows_blob"], np.float32).reshape(6, B), t_rows.numpy())
    tu = np.frombuffer(st["t_rows_unet"], np.float32).reshape(6, Bu)
    assert np.array_equal(tu[:, :B], t_rows.numpy()) and np.array_equal(tu[:, Bu - B:], t_rows.numpy())
    want = np.zeros((6, B), np.float32)
    for b, (n, s0, s1, sc) in enumerate(zip(STEPS, kw["blobnet_control_guidance_start"], kw["blobnet_control_guidance_end"],
                                            kw["blobnet_conditioning_scale"])):
        want[:n, b] = np.float32(sc) * np.array(blobnet_keep(n, s0, s1), np.float32)
    assert np.array_equal(np.frombuffer(st["scale_table"], np.float32).reshape(6, B), want)
    # another mix of values with the same (B, h, w, T, nmax, form): the same plan
    eng.compile_plan(path, B, h, w, T, D, [6, 2, 3], **dict(kw, blobnet_control_guidance_end=[0.5, 1.0, 1.0]))
    assert eng.cache_stats["plans_recorded"] == 1 and eng.cache_stats["plan_hits"] == 1
    # and a header that claims less than version 8 cannot carry the new ops
    raw = bytearray(open(path, "rb").read())
    raw[4:8] = struct.pack("<I", 7)
    (tmp_path / "v7.bcplan").write_bytes(bytes(raw))
    with pytest.raises(AssertionError, match="unknown op"):
        plan_dump(str(tmp_path / "v7.bcplan"))


def test_scalar_plans_compile_to_the_listings_and_versions_they_had(plan_dump, dump_dir, tmp_path):
    """UniPC, DDIM and Euler at one edit and at a batch of 3: file version and the whole launch listing (every non-GEMM launch with its
    arguments, every buffer with its size) are what the commit before per-request schedules wrote."""
    from blobctrl_amd.schedulers import DDIMScheduler, EulerDiscreteScheduler, UniPCMultistepScheduler
    want = json.load(open(os.path.join(GOLD, "plan_listings_before_requests.json")))
    eng = _engine()
    scheds = {"uni": UniPCMultistepScheduler(), "ddim": DDIMScheduler(), "euler": EulerDiscreteScheduler(**SD)}
    assert sorted(want) == sorted(list(scheds) + [k + "_b3" for k in scheds])
    for key in sorted(want):
        s, B = scheds[key.split("_")[0]], 3 if key.endswith("_b3") else 1
        eng.set_scheduler(s.kind, s.table_params())
        path = str(tmp_path / f"{key}.bcplan")
        eng.compile_plan(path, B, 8, 8, 7, TINY["ctx"], 6, blobnet_control_guidance_end=0.67)
        assert _version(path) == want[key]["version"], key
        r = subprocess.run([os.path.join(str(dump_dir), "plan_dump"), path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
        assert len(r.stdout.splitlines()) == want[key]["lines"], key
        assert hashlib.sha256(r.stdout.encode()).hexdigest() == want[key]["sha256"], key
    assert not any("requests" in k for k in eng._plans)


STORED = ("t_table", "t_rows_unet", "t_rows_blob", "coef", "scale_table", "freeu", "variance_noise")


def stored_table_cases():
    """name -> (scheduler object, B, compile_plan keywords): the configurations of plan_tables_before_setup_merge.json - ten scalar ones
    at B = 1 and B = 3, and the MIXED lists at B = 3, steps STEPS."""
    from blobctrl_amd.schedulers import (DDIMScheduler, DPMSolverMultistepScheduler, EulerDiscreteScheduler, HeunDiscreteScheduler,
                                         LCMScheduler, UniPCMultistepScheduler)
    cases = {}
    for B in (1, 3):
        for name, s, kw in (
                ("unipc", UniPCMultistepScheduler(), dict(num_inference_steps=6, blobnet_control_guidance_end=0.67)),
                ("ddim_eta_noise", DDIMScheduler(), dict(num_inference_steps=6, eta=0.5, variance_noise=g(7, 6, B, 4, 8, 8))),
                ("ddim_eta", DDIMScheduler(), dict(num_inference_steps=6, eta=0.5)),
                ("euler", EulerDiscreteScheduler(**SD), dict(num_inference_steps=6)),
                ("heun", HeunDiscreteScheduler(**SD), dict(num_inference_steps=4)),
                ("dpm_3m", DPMSolverMultistepScheduler(solver_order=3), dict(num_inference_steps=6)),
                ("dpm_sde", DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++"), dict(num_inference_steps=6)),
                ("lcm_single", LCMScheduler(), dict(num_inference_steps=4, guidance_scale=1.0)),
                ("unipc_freeu", UniPCMultistepScheduler(), dict(num_inference_steps=6, freeu=(0.9, 0.2, 1.2, 1.4))),
                ("dpm_timesteps", DPMSolverMultistepScheduler(), dict(num_inference_steps=None, timesteps=[999, 500, 10]))):
            cases[f"{name}_b{B}"] = (s, B, kw)
    for name, s, kw in (("ddim_eta", DDIMScheduler(), dict(MIXED, eta=[0.0, 0.5, 1.0])), ("euler", EulerDiscreteScheduler(**SD), MIXED),
                        ("lcm", LCMScheduler(), MIXED), ("lcm_single", LCMScheduler(), dict(MIXED, guidance_scale=[1.0, 1.0, 0.5]))):
        cases[f"mixed_{name}"] = (s, 3, dict(kw, num_inference_steps=list(STEPS)))
    return cases


def stored_tables(workdir):
    """name -> {"segments": what compile_plan returned, "stored": {buffer: sha256 of its stored bytes}} of every case above; a buffer the
    file keeps as workspace (a `variance_noise` nobody gave) has no entry."""
    eng, out = _engine(), {}
    for name, (s, B, kw) in stored_table_cases().items():
        eng.set_scheduler(s.kind, s.table_params())
        path = os.path.join(str(workdir), name + ".bcplan")
        seq = eng.compile_plan(path, B, 8, 8, 7, TINY["ctx"], **kw)
        st = _stored(path)
        out[name] = dict(segments=seq, stored={k: hashlib.sha256(st[k]).hexdigest() for k in STORED if k in st})
        os.remove(path)
    return out


def test_compiled_plans_store_the_tables_they_stored_before_the_setup_merge(tmp_path):
    """Scalar and list calls of compile_plan: the bytes of every table saved with its contents and the returned segment list are what
    the commit before `denoise` / `compile_plan` got their one shared set-up wrote (tools/make_plan_fixture.py --stored-tables, run
    on that commit)."""
    want = json.load(open(os.path.join(GOLD, "plan_tables_before_setup_merge.json")))
    got = stored_tables(tmp_path)
    assert sorted(got) == sorted(want) and len(want) == 24
    for name in sorted(want):
        assert got[name] == want[name], name
        names = set(got[name]["stored"])
        lists, noise = name.startswith("mixed_"), "noise" in name
        assert names - {"freeu", "variance_noise"} == ({"t_rows_unet", "t_rows_blob", "coef", "scale_table"} if lists else
                                                      {"t_table", "coef", "scale_table"}), name
        assert ("freeu" in names) == ("freeu" in name) and ("variance_noise" in names) == noise, name


# ------------------------------------------------------------------------------------------------------------ C ABI and dispatcher
def test_the_entry_points_are_exported_recordable_and_check_their_arguments():
    from blobctrl_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "blobctrl_requests.h")).read()
    assert _lib.REQUEST_OPS == {"bc_scheduler_step_requests": OP_STEP_REQUESTS, "bc_assemble_input_requests": OP_ASM_REQUESTS,
                                "bc_assemble_input_im2col_requests": OP_IM2COL_REQUESTS, "bc_timestep_embedding_rows": OP_TEMB_ROWS}
    assert set(_lib.REQUEST_OPS) == set(_lib.REQUEST_SIGNATURES) and not set(_lib.REQUEST_OPS) & set(_lib.OPS)
    for name in _lib.REQUEST_OPS:
        assert getattr(lib, name) is not None and f"int {name}(" in header and _lib.op_code(name) == _lib.REQUEST_OPS[name]
    assert _lib.op_code("bc_gemm") == 0 and _lib.op_code("bc_freeu") == 37
    assert _lib.op_signature("bc_scheduler_step_requests") == "pppppiiipiiipi"
    assert _lib.op_signature("bc_assemble_input_requests") == _lib.op_signature("bc_assemble_input_scaled")
    assert _lib.op_signature("bc_assemble_input_im2col_requests") == _lib.op_signature("bc_assemble_input_im2col_scaled")
    assert _lib.op_signature("bc_timestep_embedding_rows") == "piipip"
    # argument checks of the host wrappers: refused before anything is launched (no GPU is touched)
    p = 4096
    assert lib.bc_scheduler_step_requests(p, p, None, p, p, 3, 8, 8, None, 6, 0, 0, None, 1, None) == 1 and b"bad args" in lib.bc_last_error()
    assert lib.bc_scheduler_step_requests(p, p, p, p, p, 3, 8, 8, None, 0, 0, 0, None, 1, None) == 1
    assert lib.bc_assemble_input_requests(p, 3, p, p, None, 3, 0, 6, 8, 8, 8, 0, None, p, 6, p, None) == 1
    assert lib.bc_assemble_input_requests(p, 3, p, p, None, 3, 0, 6, 8, 8, 12, 0, p, p, 6, p, None) == 1 and b"Cpad" in lib.bc_last_error()
    assert lib.bc_assemble_input_im2col_requests(p, 3, p, p, 3, 6, 8, 8, 0, p, None, 6, p, None) == 1
    assert lib.bc_timestep_embedding_rows(None, 12, 32, None, 0, p, None) == 1 and lib.bc_timestep_embedding_rows(p, 12, 31, None, 0, p, None) == 1
    assert lib.bc_timestep_embedding_rows(p, 12, 32, p, 0, p, None) == 1


def test_denoise_requests_schema_and_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from blobctrl_amd import ops
    schema = str(torch.ops.blobctrl.denoise_requests.default._schema).replace("SymInt", "int")      # (how torch spells an int argument)
    assert schema == ("blobctrl::denoise_requests(Tensor prompt_embeds, Tensor fg_image_latents, Tensor bg_image_latents, Tensor gs_score, "
                      "Tensor dino_feats, Tensor latents, int[] num_inference_steps, float[] guidance_scale, float[] conditioning_scales, "
                      "float[] guidance_start, float[] guidance_end, int handle) -> Tensor"), schema
    assert "variance_noise=None) -> Tensor" in str(torch.ops.blobctrl.denoise.default._schema)          # (untouched)
    assert "float guidance_scale" in str(torch.ops.blobctrl.denoise.default._schema)
    eng = _engine()
    a = _batch(3)
    with FakeTensorMode() as mode:
        fake = {k: mode.from_tensor(v) for k, v in a.items()}
        out = torch.ops.blobctrl.denoise_requests(fake["prompt_embeds"], fake["fg_image_latents"], fake["bg_image_latents"], fake["gs_score"],
                                                  fake["dino_feats"], fake["latents"], [4, 6, 5], [7.5, 3.0, 1.0], [1.0, 0.0, 1.7],
                                                  [0.0, 0.2, 0.0], [1.0, 0.7, 0.5], ops.register(eng))
        assert tuple(out.shape) == (3, 4, 8, 8) and out.dtype == torch.float32 and out.device == eng.device
    assert eng.cache_stats["plans_recorded"] == 0
