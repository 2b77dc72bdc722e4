"""Stochastic DDIM (eta > 0) without a GPU: the coefficient tables and the drop-in scheduler against the reference's DDIMScheduler.step
(tests/golden/schedulers_eta.npz), the noise-drawing helper against the noise the reference drew (loop_tiny_eta.npz,
pipeline_call_eta.npz), and what a compiled stochastic plan launches (read back through the host-side `.bcplan` parser)."""
import os

import numpy as np
import pytest
import torch

from tests.common import TINY, build_plan_dump, g, plan_named as _named, plan_stored, tiny_weights

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
OP_STEP, OP_STEP_NOISE = 11, 30


def _gold(name):
    return np.load(os.path.join(GOLD, name))


def _table_traj(n, eta, noise_seed=200):
    from blobctrl_amd.schedulers import DDIMTable, apply_table_step
    tab = DDIMTable().set_timesteps(n, eta=eta)
    x = g(21, 1, 4, 8, 8)
    z = torch.zeros_like(x)
    hist = dict(m0=z, m1=z.clone(), last=z.clone())
    xs = [x]
    for i in range(n):
        x = apply_table_step(tab.coef[i].tolist(), g(100 + i, 1, 4, 8, 8), x, hist, noise=g(noise_seed + i, 1, 4, 8, 8))
        xs.append(x)
    return torch.stack(xs).numpy()


@pytest.mark.parametrize("n", [5, 20, 50])
@pytest.mark.parametrize("eta", [0.3, 1.0])
def test_table_rows_reproduce_the_reference_eta_trajectories(n, eta):
    ref = _gold("schedulers_eta.npz")[f"ddim_{n}_eta{int(round(eta * 10)):02d}_traj"]
    got = _table_traj(n, eta)
    assert got.shape == ref.shape
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())


def test_eta_zero_rows_are_the_deterministic_rows():
    from blobctrl_amd.schedulers import DDIMTable
    for n in (5, 20, 50):
        tab = DDIMTable().set_timesteps(n)
        assert torch.equal(DDIMTable().set_timesteps(n, eta=0.0).coef, tab.coef)
        assert (tab.coef[:, 12] == 0).all() and (tab.coef[:, 11] == 0).all()
        # the rows as tabulated before eta existed: columns 0, 1, 8, 10 only
        ac = tab.alphas_cumprod
        ratio = 1000 // n
        for i, t in enumerate(tab.timesteps.tolist()):
            a_t = ac[t]
            a_prev = ac[t - ratio] if t - ratio >= 0 else ac[0]
            row = torch.zeros(16)
            row[0], row[1] = 1.0 / a_t ** 0.5, (1 - a_t) ** 0.5 / a_t ** 0.5
            row[8], row[10] = a_prev ** 0.5, (1 - a_prev) ** 0.5
            assert torch.equal(tab.coef[i], row), (n, i)
        stoch = DDIMTable().set_timesteps(n, eta=1.0).coef
        assert (stoch[:, 12] > 0).all() and (stoch[:, 10] < tab.coef[:, 10]).all()
        assert torch.equal(stoch[:, [0, 1, 8]], tab.coef[:, [0, 1, 8]])


def test_dropin_ddim_step_honours_eta_generator_and_variance_noise():
    from blobctrl_amd.schedulers import DDIMScheduler
    z = _gold("schedulers_eta.npz")

    def run(n, kw_of_step):
        s = DDIMScheduler()
        s.set_timesteps(n)
        x = g(21, 1, 4, 8, 8)
        xs = [x]
        for i, t in enumerate(s.timesteps):
            kw = kw_of_step(i)
            out = s.step(g(100 + i, 1, 4, 8, 8), t, x, **kw)
            x = out[0] if isinstance(out, tuple) else out.prev_sample
            xs.append(x)
        return torch.stack(xs).numpy()

    for n in (5, 20):
        for eta in (0.3, 1.0):
            ref = z[f"ddim_{n}_eta{int(round(eta * 10)):02d}_traj"]
            got = run(n, lambda i: dict(eta=eta, variance_noise=g(200 + i, 1, 4, 8, 8), return_dict=False))
            np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    gen = torch.Generator().manual_seed(77)
    ref = z["ddim_5_eta10_gen77_traj"]
    got = run(5, lambda i: dict(eta=1.0, generator=gen))
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    assert run(5, lambda i: dict(eta=0.7, generator=torch.Generator().manual_seed(77))).shape == ref.shape
    # eta = 0 is the deterministic update whatever noise is passed (the reference adds noise only for eta > 0)
    base = run(5, lambda i: dict(return_dict=False))
    assert np.array_equal(base, run(5, lambda i: dict(eta=0.0, variance_noise=g(200 + i, 1, 4, 8, 8))))
    assert not np.allclose(base, ref)
    s = DDIMScheduler()
    s.set_timesteps(5)
    x = g(21, 1, 4, 8, 8)
    with pytest.raises(ValueError, match="Cannot pass both generator and variance_noise"):
        s.step(x, s.timesteps[0], x, eta=1.0, generator=torch.Generator(), variance_noise=torch.zeros_like(x))
    with pytest.raises(ValueError, match="step"):                     # 1 - alpha_prev - std^2 < 0: no finite update
        s.step(x, s.timesteps[0], x, eta=5.0)
    from blobctrl_amd.schedulers import DDIMTable
    with pytest.raises(ValueError, match="step"):
        DDIMTable().set_timesteps(50, eta=5.0)


def test_noise_helper_draws_exactly_what_the_reference_drew():
    from blobctrl_amd.pipeline import BlobCtrlEngine
    draw = BlobCtrlEngine.variance_noise
    z = _gold("loop_tiny_eta.npz")
    for tag in ("ddim_5", "ddim_6"):
        ref = z[f"{tag}_noise"]                                        # [steps, 1, 4, 8, 8], tapped from scheduler.step
        got = draw(ref.shape[0], 1, 8, 8, torch.Generator().manual_seed(int(z[f"{tag}_seed"])), device="cpu")
        assert got.dtype == torch.float32 and np.array_equal(got.numpy(), ref), tag
        got1 = draw(ref.shape[0], 1, 8, 8, [torch.Generator().manual_seed(int(z[f"{tag}_seed"]))], device="cpu")   # one-element list
        assert np.array_equal(got1.numpy(), ref)
    # a list of generators: one sample per generator and step (the reference's randn_tensor, three generators)
    ref = z["list3_noise"]
    got = draw(2, 3, 8, 8, [torch.Generator().manual_seed(int(s)) for s in z["list3_seeds"]], device="cpu")
    assert np.array_equal(got.numpy(), ref)
    # B = 3 with one generator: one [3, 4, h, w] draw per step
    gen, chk = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    got = draw(4, 3, 8, 8, gen, device="cpu")
    assert got.shape == (4, 3, 4, 8, 8)
    assert all(torch.equal(got[i], torch.randn((3, 4, 8, 8), generator=chk)) for i in range(4))
    with pytest.raises(ValueError):
        draw(2, 3, 8, 8, [torch.Generator(), torch.Generator()], device="cpu")
    # __call__ order: the generator draws the start latents first (prepare_latents), then every step's noise
    zc = _gold("pipeline_call_eta.npz")
    gen = torch.Generator().manual_seed(int(zc["seed"]))
    B = zc["latents"].shape[0]
    torch.randn((B, 4, 8, 8), generator=gen, dtype=torch.float32)
    got = draw(zc["noise"].shape[0], B, 8, 8, gen, device="cpu")
    assert np.array_equal(got.numpy(), zc["noise"])


# ------------------------------------------------------------------------------------------------------------ compiled plans
@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    return build_plan_dump(tmp_path_factory.mktemp("dump"))


@pytest.fixture(scope="module")
def ddim_engine():
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from tests.gpu_common import tiny_trunk_configs
    usd, bsd = tiny_weights()
    ucfg, bcfg = tiny_trunk_configs()
    return BlobCtrlEngine(usd, bsd, ucfg, bcfg, device="cpu", scheduler="ddim", compile_only=True)


def test_compiled_plans_launch_the_noise_step_only_when_stochastic(ddim_engine, plan_dump, tmp_path):
    n, B, h, w, T = 5, 1, 8, 8, 7
    noise = g(77, n, B, 4, h, w)
    det, sto = str(tmp_path / "det.bcplan"), str(tmp_path / "sto.bcplan")
    seq0 = ddim_engine.compile_plan(det, B, h, w, T, TINY["ctx"], n)
    seq1 = ddim_engine.compile_plan(sto, B, h, w, T, TINY["ctx"], n, eta=1.0, variance_noise=noise)
    assert seq0 == seq1 == ["step_active"] * n
    # eta = 0: no noise op, no noise buffer; each step segment still ends in today's bc_cfg_scheduler_step launch
    bufs, segs = plan_dump(det)
    assert "variance_noise" not in {nm for nm, _ in bufs.values()}
    for name in ("step_active", "step_inactive"):
        ops = [op for op, _, _ in segs[name]]
        assert OP_STEP_NOISE not in ops and ops.count(OP_STEP) == 1 and ops[-1] == OP_STEP, name
        a = segs[name][-1][2]
        assert [_named(bufs, a[k]) for k in (1, 2, 3, 4, 9)] == [("latents", 0), ("coef", 0), ("step_idx", 0), ("hist", 0),
                                                                  ("eps_guided", 0)]
        assert a[5:9] == ["-1", "1", "8", "8"] and a[10] == "1"
    assert not {OP_STEP, OP_STEP_NOISE} & {op for op, _, _ in segs["prologue"]}
    # eta > 0: exactly one noise op per step segment, in place of the deterministic one, reading the named noise buffer
    bufs1, segs1 = plan_dump(sto)
    named = {nm: (i, nb) for i, (nm, nb) in bufs1.items()}
    assert named["variance_noise"][1] == n * B * 4 * h * w * 4
    for name in ("step_active", "step_inactive"):
        ops = [op for op, _, _ in segs1[name]]
        assert ops.count(OP_STEP_NOISE) == 1 and OP_STEP not in ops and ops[-1] == OP_STEP_NOISE, name
        a = segs1[name][-1][2]
        assert len(a) == 13                                              # "pppppfiiipipi"
        assert [_named(bufs1, a[k]) for k in (1, 2, 3, 4, 9, 11)] == [("latents", 0), ("coef", 0), ("step_idx", 0), ("hist", 0),
                                                                       ("variance_noise", 0), ("eps_guided", 0)]
        assert a[5:9] == ["-1", "1", "8", "8"] and a[10] == str(n) and a[12] == "1"
        assert len(segs1[name]) == len(segs[name])                      # the same launch list otherwise
    # the noise is stored WITH its contents (a C host can run the edit as is, or refill the named buffer)
    data = plan_stored(sto)
    assert np.array_equal(np.frombuffer(data["variance_noise"], np.float32), noise.numpy().reshape(-1))
    coef = np.frombuffer(data["coef"], np.float32).reshape(n, 16)
    from blobctrl_amd.schedulers import DDIMTable
    assert np.array_equal(coef[:, :11], DDIMTable().set_timesteps(n, eta=1.0).coef.numpy()[:, :11]) and (coef[:, 12] > 0).all()
    # without noise contents the buffer is plain (zero-filled) workspace for the host to fill
    bare = str(tmp_path / "bare.bcplan")
    ddim_engine.compile_plan(bare, B, h, w, T, TINY["ctx"], n, eta=0.5)
    bufs2, _ = plan_dump(bare)
    assert "variance_noise" in {nm for nm, _ in bufs2.values()}
    assert os.path.getsize(bare) < os.path.getsize(sto)


def test_eta_arguments_are_checked_without_a_gpu(ddim_engine, tmp_path):
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from tests.gpu_common import tiny_trunk_configs
    path = str(tmp_path / "x.bcplan")
    with pytest.raises(NotImplementedError):
        ddim_engine.compile_plan(path, 1, 8, 8, 7, TINY["ctx"], 5, eta=-0.5)
    with pytest.raises(ValueError):
        ddim_engine.compile_plan(path, 1, 8, 8, 7, TINY["ctx"], 5, eta=1.0, variance_noise=torch.zeros(4, 1, 4, 8, 8))
    with pytest.raises(ValueError, match="step"):
        ddim_engine.compile_plan(path, 1, 8, 8, 7, TINY["ctx"], 5, eta=5.0)
    usd, bsd = tiny_weights()
    ucfg, bcfg = tiny_trunk_configs()
    uni = BlobCtrlEngine(usd, bsd, ucfg, bcfg, device="cpu", scheduler="unipc", compile_only=True)
    with pytest.raises(NotImplementedError, match="DDIM"):
        uni.compile_plan(path, 1, 8, 8, 7, TINY["ctx"], 5, eta=0.5)


def test_denoise_op_schema_takes_eta_and_variance_noise():
    from blobctrl_amd import ops  # noqa: F401
    schema = str(torch.ops.blobctrl.denoise.default._schema)
    assert "float eta=0." in schema and "Tensor? variance_noise=None" in schema and schema.endswith("-> Tensor")
