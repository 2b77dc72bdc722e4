"""Masked edits on the host: the symbol and op tables, the argument refusals of both entry points, PlanSpec / EditPlan with `blend`, the
refusals, `blend_rows()` of every table against the reference's add_noise (tests/golden/pipeline_call_blend.npz), the float64
restatement of tests/blend_common.py against the reference's blended steps, its power, and the host mask path (blend_mask.npz)."""
import inspect
import os

import numpy as np
import pytest
import torch

from tests import blend_common as bc
from tests.common import TINY, tiny_weights
from tests.gpu_common import tiny_trunk_configs

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000, steps_offset=1)
TABLE_BAR = 5e-6                        # of max |reference|: the bar of the scheduler-table tests (test_host_cpu.py, test_dpm_solver_cpu.py)


@pytest.fixture(scope="module")
def zb():
    return np.load(os.path.join(GOLD, "pipeline_call_blend.npz"))


def _engine(**kw):
    from blobctrl_amd.pipeline import BlobCtrlEngine
    usd, bsd = tiny_weights()
    ucfg, bcfg = tiny_trunk_configs()
    return BlobCtrlEngine(usd, bsd, ucfg, bcfg, device="cpu", scheduler="ddim", compile_only=True, max_cached_plans=16, **kw)


def _table(eng, case):
    """The coefficient table the engine builds for a fixture case."""
    from blobctrl_amd import schedulers
    extra = bc.BLEND_CASES[case]
    s = bc.make_scheduler(schedulers, extra["scheduler"], SD)
    eng.set_scheduler(s.kind, s.table_params())
    return eng._scheduler_table(extra.get("num_inference_steps", bc.BLEND_STEPS), extra.get("eta", 0.0))


# ---------------------------------------------------------------------------------------------------- symbols and ops
def test_blend_symbols_resolve_and_their_ops_stand_behind_the_pag_enum(tmp_path):
    import ctypes as C
    from blobctrl_amd import _lib
    lib = _lib.load()
    assert set(_lib.BLEND_SIGNATURES) == set(_lib.BLEND_OPS) and _lib.BLEND_OPS == {"bc_blend_scheduler_step": 63, "bc_blend_mask": 64}
    assert _lib._OP_TABLES_BLEND == (_lib.BLEND_OPS,) and _lib._OP_TABLES_PAG == (_lib.PAG_OPS,) and len(_lib.EXPORTED_SYMBOLS) == 92
    for name, code in _lib.BLEND_OPS.items():
        assert getattr(lib, name) is not None and name not in _lib.EXPORTED_SYMBOLS and _lib.op_code(name) == code
        assert not any(name in t for t in _lib._OP_TABLES + _lib._OP_TABLES_BEYOND + _lib._OP_TABLES_TINY_VAE + _lib._OP_TABLES_PAG)
    assert _lib.op_signature("bc_blend_scheduler_step") == "ppppppppppiiipiiipi" and _lib.op_signature("bc_blend_mask") == "ppiii"
    assert _lib.op_signature("bc_pag_scheduler_step") == "ppppppiiipiiipi"
    header = open(os.path.join(os.path.dirname(GOLD), "..", "include", "blobctrl_blend.h")).read()
    assert '#include "blobctrl_pag.h"' in header and "BC_OP_BLEND_SCHEDULER_STEP = BC_OP_PAG_END + 1, BC_OP_BLEND_MASK, BC_OP_BLEND_END" in header
    plan = C.c_void_p()
    assert lib.bc_plan_create(C.byref(plan)) == 0
    try:
        seg = lib.bc_plan_segment(plan, b"s")
        words = (C.c_uint64 * 20)()
        assert lib.bc_plan_add_op(plan, seg, 0, 63, words, 19) == 0 and lib.bc_plan_add_op(plan, seg, 0, 64, words, 5) == 1
        assert lib.bc_plan_add_op(plan, seg, 0, 63, words, 18) < 0 and b"op 63 takes 19" in lib.bc_last_error()
        assert lib.bc_plan_add_op(plan, seg, 0, 64, words, 6) < 0
        for n in (5, 19):                                                  # 62 (BC_OP_PAG_END) and 65 (BC_OP_BLEND_END) are no ops
            assert lib.bc_plan_add_op(plan, seg, 0, 62, words, n) < 0 and lib.bc_plan_add_op(plan, seg, 0, 65, words, n) < 0
        buf = (_lib.BcPlanBuffer * 1)()
        buf[0].name, buf[0].address, buf[0].bytes = b"x", 0x1000, 16
        path = str(tmp_path / "blend.bcplan")
        assert lib.bc_plan_save(plan, path.encode(), buf, 1) != 0 and b"in-process only" in lib.bc_last_error() and not os.path.exists(path)
    finally:
        lib.bc_plan_destroy(plan)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Argument checks come before the launch, so they run without a device."""
    from blobctrl_amd import _lib
    lib = _lib.load()
    a = 1 << 20                                                                    # (an address that is never dereferenced)
    good = [a, a, a, a, a, None, a, a, a, a, 1, 2, 2, None, 3, 0, 0, a, 1]
    for k, v in ((0, None), (1, None), (2, None), (3, None), (4, None), (6, None), (7, None), (8, None), (9, None), (10, 0), (11, 0),
                 (12, -1), (14, 0), (10, 1 << 29)):
        args = list(good)
        args[k] = v
        assert lib.bc_blend_scheduler_step(*args, None) == 1 and b"bc_blend_scheduler_step" in lib.bc_last_error(), (k, v)
    for args in ((None, a, 1, 8, 8), (a, None, 1, 8, 8), (a, a, 0, 8, 8), (a, a, 1, 12, 8), (a, a, 1, 8, 20), (a, a, 1, 0, 8),
                 (a, a, 1 << 12, 1 << 10, 1 << 10)):
        assert lib.bc_blend_mask(*args, None) == 1 and b"bc_blend_mask" in lib.bc_last_error(), args


# ---------------------------------------------------------------------------------------------------- PlanSpec and the plan
def test_plan_spec_gains_blend_last_and_the_plan_owns_its_buffers():
    from blobctrl_amd import pag
    from blobctrl_amd.edit_plan import PlanSpec
    from blobctrl_amd.pipeline import BlobCtrlEngine, EditSetup
    eng = _engine()
    mid = pag.resolve_layers(eng.unet_cfg, "mid")
    base = dict(B=2, h=8, w=8, T=7, ctx_dim=TINY["ctx"], nsteps=3)
    for kw in (dict(), dict(stochastic=True), dict(third_order=True, scaled=True), dict(single=True, freeu=True), dict(pag=mid)):
        plain, on = PlanSpec(**base, **kw), PlanSpec(**base, **kw, blend=1)
        assert plain.blend is False and on.blend is True and on.key() == plain.key() + ("blend",) and "blend" not in plain.key()
        name, head, tail = on.step_call()
        assert name == "bc_blend_scheduler_step" and head == ("pag_table", "blend_image", "blend_noise", "blend_mask", "blend_table")
        assert tail == ("variance_noise", 3, int(on.third_order), int(on.single)) and plain.step_call()[0] != name
    assert list(inspect.signature(BlobCtrlEngine.plan_for).parameters)[-1] == "pag"           # (plan_for keeps its parameter list)
    assert "blend" in inspect.signature(EditSetup.plan_spec).parameters
    P0 = eng.plan_for(2, 8, 8, 7, TINY["ctx"], 3)
    assert all(getattr(P0, n) is None for n in ("blend_image", "blend_noise", "blend_mask", "blend_table"))
    ident = lambda P: [[(r[0], r[1], len(r[2])) for r in seg.recs] if hasattr(seg, "recs") else [m["kind"] for m in seg.meta]
                       for seg in (P.prologue, P.step_active, P.step_inactive)]
    for kw in (dict(), dict(pag=mid)):
        other = eng._plan(PlanSpec(**base, **kw))
        P = eng._plan(PlanSpec(**base, **kw, blend=True))
        assert list(eng._plans)[-1][-1] == "blend"
        assert P.blend_image.shape == P.blend_noise.shape == (2, 4, 8, 8) and P.blend_mask.shape == (2, 8, 8) and P.blend_table.shape == (3, 2)
        for n in ("blend_image", "blend_noise", "blend_mask", "blend_table"):
            assert P.rec.named[n] is getattr(P, n) and getattr(P, n).dtype == torch.float32
        assert (P.pag_table is None) == (not kw)
        for seg, oseg in ((P.step_active, other.step_active), (P.step_inactive, other.step_inactive)):
            kinds, okinds = [m["kind"] for m in seg.meta], [m["kind"] for m in oseg.meta]
            assert kinds == okinds and kinds[-1] == "cfg_step"                     # the same launches; only the step's entry point differs
    assert ident(eng.plan_for(2, 8, 8, 7, TINY["ctx"], 3)) == ident(P0)


def test_refusals_say_why():
    from blobctrl_amd.edit_plan import PlanSpec
    eng = _engine()
    args = lambda B=1: (torch.zeros(2 * B, 7, TINY["ctx"]), torch.zeros(B, 4, 8, 8), torch.zeros(B, 4, 8, 8), torch.zeros(B, 2, 8, 8),
                        torch.zeros(B, 1, TINY["feat"]))
    img, m = torch.zeros(1, 4, 8, 8), torch.ones(1, 1, 8, 8)
    with pytest.raises(NotImplementedError, match="ONE blend_table"):
        PlanSpec(2, 8, 8, 7, TINY["ctx"], 3, per_request=True, requests=True, blend=True).validate()
    with pytest.raises(NotImplementedError, match="per-request schedules"):
        eng.denoise(*args(2), num_inference_steps=[2, 3], latents=torch.zeros(2, 4, 8, 8), blend_image_latents=img, blend_mask=m)
    for kw in (dict(blend_image_latents=img), dict(blend_mask=m)):
        with pytest.raises(ValueError, match="both or neither"):
            eng.denoise(*args(), latents=torch.zeros(1, 4, 8, 8), **kw)
    for kw in (dict(blend_image_latents=torch.zeros(1, 4, 8, 9), blend_mask=m), dict(blend_image_latents=img, blend_mask=torch.ones(1, 1, 8, 9)),
               dict(blend_image_latents=torch.zeros(3, 4, 8, 8), blend_mask=m), dict(blend_image_latents=img, blend_mask=torch.ones(1, 8, 8, dtype=torch.int32))):
        with pytest.raises(ValueError, match="blend_"):
            eng.denoise(*args(), latents=torch.zeros(1, 4, 8, 8), num_inference_steps=3, **kw)
    eng.set_scheduler("heun")
    with pytest.raises(NotImplementedError, match="second stage"):
        eng.denoise(*args(), latents=torch.zeros(1, 4, 8, 8), num_inference_steps=3, blend_image_latents=img, blend_mask=m)
    eng.set_scheduler("ddim")
    with pytest.raises(NotImplementedError, match="in-process only"):
        eng.compile_plan("/nonexistent/x.bcplan", 1, 8, 8, 7, TINY["ctx"], 3, blend_image_latents=img, blend_mask=m)
    assert not eng._plans                                                          # nothing was recorded on the way to a refusal
    from blobctrl_amd.pipeline import StableDiffusionBlobNetPipeline as Pipe
    sig = inspect.signature(Pipe.__call__).parameters
    assert sig["image"].default is None and sig["mask_image"].default is None
    p = Pipe.__new__(Pipe)
    p.vae_scale_factor = 8
    for kw in (dict(image=img, mask_image=None), dict(image=None, mask_image=np.zeros((64, 64), np.uint8))):
        with pytest.raises(ValueError, match="go together"):
            p._check_blend_inputs(height=64, width=64, **kw)
    with pytest.raises(ValueError, match="divisible by 8"):
        p._check_blend_inputs(img, np.zeros((60, 64), np.uint8), 60, 64)
    with pytest.raises(ValueError, match="exactly"):
        p._check_blend_inputs(img, torch.zeros(32, 64, dtype=torch.uint8), 64, 64)
    p._check_blend_inputs(None, None, 60, 64)


# ---------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("case", list(bc.BLEND_CASES))
def test_blend_rows_are_the_reference_add_noise_coefficients(zb, case):
    tab = _table(_engine(), case)
    rows, ref = tab.blend_rows(), zb[f"{case}_add_noise"]
    assert rows.dtype == torch.float32 and tuple(rows.shape) == ref.shape == (len(tab.timesteps), 2)
    assert np.array_equal(np.asarray(tab.timesteps, dtype=np.float64), zb[f"{case}_timesteps"].astype(np.float64))
    assert rows[-1].tolist() == [1.0, 0.0] and ref[-1].tolist() == [1.0, 0.0]
    err = np.abs(rows.numpy().astype(np.float64) - ref).max(0)
    print(f"blend_rows {case}: max-abs error (a, s) {err}, reference max {np.abs(ref).max(0)}")
    assert (err <= TABLE_BAR * np.abs(ref).max(0)).all(), (case, err)
    if bc.BLEND_CASES[case]["scheduler"] in ("euler", "eulera"):
        assert (rows[:-1, 0] == 1).all() and np.array_equal(rows[:-1, 1].numpy(), tab.sigmas[1:-1].numpy())


def test_heun_has_no_blend_rows():
    from blobctrl_amd.schedulers import HeunTable
    with pytest.raises(NotImplementedError, match="second stage"):
        HeunTable().set_timesteps(3).blend_rows()


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("case", list(bc.BLEND_CASES))
def test_the_float64_blended_step_follows_the_reference_loop(zb, case):
    """tests/blend_common.py's step + blend from the engine's own tables on the reference's guided eps and the sample entering every
    step: the blended latents leaving it, at the bar of the scheduler-table tests, and exactly the image outside the mask at the end."""
    tab = _table(_engine(), case)
    eps, x_in, x_out = (torch.from_numpy(zb[f"{case}_step_{k}"]) for k in ("eps", "in", "out"))
    n, B = eps.shape[0], eps.shape[1]
    lat, image, mask = bc.blend_inputs(B)
    noise = torch.from_numpy(zb[f"{case}_step_noise"]) if f"{case}_step_noise" in zb.files else None
    rows, third = tab.blend_rows(), bool((tab.coef[:, 13] != 0).any())
    hist = torch.zeros(3, x_in[0].numel(), dtype=torch.float64)
    assert np.array_equal(x_in[0].numpy(), (lat * tab.init_noise_sigma).numpy())
    worst = 0.0
    for i in range(n):
        nz = noise[i] if noise is not None and i < noise.shape[0] else None
        xn, hist = bc.host_step(tab.coef[i], eps[i], x_in[i], hist, nz, third)
        got = bc.blend(xn, image, lat, mask[0].expand(B, 8, 8), rows[i])
        err = float((got - x_out[i].double()).abs().max() / x_out[i].abs().max())
        worst = max(worst, err)
        assert err <= TABLE_BAR, (case, i, err)
        if i + 1 < n:
            assert np.array_equal(x_in[i + 1].numpy(), x_out[i].numpy())           # the loop went on from the blended latents
    print(f"blended step {case}: worst max-abs / max |reference| over {n} steps {worst:.3e}")
    keep = (mask[0] == 0).expand(B, 4, 8, 8)
    assert np.array_equal(zb[f"{case}_blend_latents"][keep.numpy()], image.numpy()[keep.numpy()])
    assert np.array_equal(zb[f"{case}_blend_latents"], x_out[-1].numpy())


@pytest.mark.parametrize("shape", bc.STEP_SHAPES)
@pytest.mark.parametrize("form", bc.STEP_FORMS)
def test_the_restatement_tells_the_wrong_launches_apart(shape, form):
    """Each wrong launch of the issue's table moves most blended elements of the test inputs outside the step bar."""
    for single in (False, True):
        for pag in (False, True):
            power = bc.step_power(bc.step_inputs(shape, form, single, pag), form, single)
            assert set(power) == set(bc.WRONG_LAUNCHES) - (set() if form == "noise" else {"blend order"})
            assert min(power.values()) > 0.5, (shape, form, single, pag, power)


# ---------------------------------------------------------------------------------------------------- the host mask path
def test_host_mask_path_is_the_reference_mask_processor_and_nearest_reduction():
    from PIL import Image
    from blobctrl_amd.pipeline import StableDiffusionBlobNetPipeline as Pipe
    z = np.load(os.path.join(GOLD, "blend_mask.npz"))
    m8 = z["mask_u8"]
    assert (m8[::8, ::8] == 127).any() and (m8[::8, ::8] == 128).any()
    p = Pipe.__new__(Pipe)
    p.vae_scale_factor = 8
    for given in (Image.fromarray(m8), m8):
        got = p.prepare_blend_mask(given, 48, 72, 1)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy(), z["mask_latent"])
    assert np.array_equal(z["mask_latent"][0, 0], (m8[::8, ::8] >= 128).astype(np.float32))       # the rule bc_blend_mask states
    with pytest.raises(ValueError, match="required batch size"):
        p.prepare_blend_mask([m8, m8, m8], 48, 72, 2)
