"""Perturbed-attention guidance on the host: the layer-matching rule and the scale table against what the reference's PAGMixin gives
(tests/golden/unet_tiny_pag.npz), the float64 restatements of tests/pag_common.py against the reference's blocks (blocks_pag.npz), the
plan keys and launch lists with and without PAG, the refusals, and the symbol and op tables."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests import pag_common as pc
from tests.common import TINY, tiny_weights
from tests.gpu_common import tiny_trunk_configs

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def zu():
    return np.load(os.path.join(GOLD, "unet_tiny_pag.npz"))


def _engine(**kw):
    from blobctrl_amd.pipeline import BlobCtrlEngine
    usd, bsd = tiny_weights()
    ucfg, bcfg = tiny_trunk_configs()
    return BlobCtrlEngine(usd, bsd, ucfg, bcfg, device="cpu", scheduler="ddim", compile_only=True, max_cached_plans=16, **kw)


# ---------------------------------------------------------------------------------------------------- layer resolution
def test_layer_ids_match_the_modules_the_reference_matches(zu):
    from blobctrl_amd import pag
    ucfg = tiny_trunk_configs()[0]
    ids = json.loads(str(zu["match_ids"]))
    assert tuple(ids) == pc.PAG_MATCH_IDS
    unmatched = 0
    for i, layer_id in enumerate(ids):
        want = json.loads(str(zu[f"match_{i}"]))
        if not want:
            unmatched += 1
            with pytest.raises(ValueError, match="Cannot find PAG layer"):
                pag.matched_names(ucfg, layer_id)
            with pytest.raises(ValueError, match="Cannot find PAG layer"):
                pag.resolve_layers(ucfg, ["mid", layer_id])
            continue
        assert pag.matched_names(ucfg, layer_id) == want, layer_id
        assert pag.resolve_layers(ucfg, layer_id) == tuple(sorted(n[: -len("transformer_blocks.0.attn1")] for n in want))
    assert unmatched == 1
    for case, layers in pc.PAG_UNET_LAYERS.items():
        want = json.loads(str(zu[f"names_{case}"]))
        assert pag.resolve_layers(ucfg, layers) == tuple(sorted(n[: -len("transformer_blocks.0.attn1")] for n in want)), case
    # the full-size UNet has the same 16 self-attentions; "mid" is one block, the issue's ids all resolve
    from blobctrl_amd.engine import TrunkConfig
    full = TrunkConfig(in_channels=5)
    assert len(pag.self_attention_names(full)) == 16 and pag.resolve_layers(full, "mid") == ("mid_block.attentions.0.",)
    assert [len(pag.resolve_layers(full, i)) for i in ("down", "up", "down_blocks.1", "up_blocks.(1|2)")] == [6, 9, 2, 6]


@pytest.mark.parametrize("bad", [3, None, ["mid", 1.5], ("mid",)])
def test_layers_that_are_no_strings_are_a_value_error(bad):
    from blobctrl_amd import pag
    with pytest.raises(ValueError, match="Expected either a string or a list of string"):
        pag.normalize_layers(bad)


def test_fake_integral_matches_are_excluded():
    """`is_fake_integral_match`: an id and a name that END in the same number.  No attn1 name of a UNet ends in one, so the rule is
    exercised on the function itself."""
    from blobctrl_amd.pag import _is_fake_integral_match
    assert _is_fake_integral_match("blocks.1", "transformer_blocks.1") and not _is_fake_integral_match("blocks.1", "transformer_blocks.10")
    assert not _is_fake_integral_match("blocks.1", "transformer_blocks.0.attn1") and not _is_fake_integral_match("mid", "mid")


# ---------------------------------------------------------------------------------------------------- pag_table
def test_pag_table_equals_get_pag_scale(zu):
    from blobctrl_amd import pag
    for case, (s, a) in pc.PAG_SCALE_CASES.items():
        got = np.array(pag.pag_table(pc.PAG_SCALE_TIMESTEPS, s, a))
        assert np.array_equal(got, zu[f"scale_{case}"]), (case, got, zu[f"scale_{case}"])
    assert min(pag.pag_table(pc.PAG_SCALE_TIMESTEPS, *pc.PAG_SCALE_CASES["clamped"])) == 0.0
    assert pag.is_active(3.0, ("x",)) and not pag.is_active(0.0, ("x",)) and not pag.is_active(3.0, ()) and not pag.is_active(3.0, None)


def test_write_tables_fills_one_row_per_evaluation():
    """`_write_tables` on a DDIM and on a Heun set-up: pag_table holds _get_pag_scale of every evaluation's timestep - Heun has 2 n - 1."""
    from blobctrl_amd import pag, schedulers
    eng = _engine()
    prefixes = pag.resolve_layers(eng.unet_cfg, "mid")
    for kind, steps, evals in (("ddim", 3, 3), ("heun", 3, 5)):
        if kind == "heun":
            s = schedulers.HeunDiscreteScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000)
            eng.set_scheduler(s.kind, s.table_params())
        S = eng._setup(1, False, 1.0, [1.0], steps, None, 5.0, 0.0, 1.0, 0.0, False)
        assert S.n == evals
        P = eng.plan_for(1, 8, 8, 7, TINY["ctx"], S.n, scaled=S.scaled, pag=prefixes)
        written = eng._write_tables(P, S, None, (3.0, 0.004))
        ts = S.t_rows[:, 0].tolist()
        want = torch.clamp(3.0 - 0.004 * (1000 - torch.tensor(ts, dtype=torch.float32)), min=0.0)       # (float32, as the reference evaluates it)
        assert P.pag_table.shape == (evals,) and torch.equal(P.pag_table, want) and any(w is P.pag_table for w in written)
        assert len(set(P.pag_table.tolist())) == evals or kind == "heun"
        eng._write_tables(P, S, None, (1.5, 0.0))
        assert torch.equal(P.pag_table, torch.full((evals,), 1.5))


# ---------------------------------------------------------------------------------------------------- the float64 restatement
@pytest.mark.parametrize("name", sorted(pc.PAG_BLOCK_CASES))
def test_float64_block_reproduces_the_reference_block(name):
    """pag_common.pag_block_reference - the checker of the GPU tests - against the reference's Transformer2DModel with the PAG processor on
    attn1, to fp32 rounding (the reference computes in fp32: 1e-4 of the output's scale), and 10 bars away from the unperturbed block."""
    z = np.load(os.path.join(GOLD, "blocks_pag.npz"))
    p = pc.PAG_BLOCK_CASES[name]
    x, ctx = pc.pag_block_inputs(name)
    n = p["B"] // p["chunks"]
    assert torch.equal(x[-n:], x[-2 * n:-n]) and torch.equal(ctx[-n:], ctx[-2 * n:-n])
    sd = pc.pag_block_weights(name)
    got = pc.pag_block_reference(sd, x, ctx, p["heads"], n_perturbed=n).numpy()[:, :, ::p["sub"], ::p["sub"]]
    ref = z[name]
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"float64 PAG block {name}: max-abs/scale vs the reference {err:.2e}")
    assert got.shape == ref.shape and err < 1e-4
    plain = pc.pag_block_reference(sd, x, ctx, p["heads"], n_perturbed=0).numpy()[:, :, ::p["sub"], ::p["sub"]]
    assert np.abs(plain[:-n] - ref[:-n]).max() / np.abs(ref).max() < 1e-4               # the other images are what they were
    assert np.abs(plain[-n:] - ref[-n:]).max() >= 10 * 1e-2 * np.abs(ref).max()          # a missing perturbation shows
    assert np.abs(ref[-n:] - ref[-2 * n:-n]).max() >= 10 * 1e-2 * np.abs(ref).max()


def test_guidance_restatement_on_numbers_worked_by_hand():
    """pag_utils.py `_apply_perturbed_attention_guidance` on e_u = 1, e_c = 2, e_p = 0.5 (second image: -1, 0.5, 2), g = 7.5, s = 3:
    1 + 7.5 (2 - 1) + 3 (2 - 0.5) = 13 and -1 + 7.5 * 1.5 + 3 * (-1.5) = 5.75; without CFG 2 + 3 * 1.5 = 6.5 and 0.5 - 4.5 = -4."""
    e = torch.tensor([[1.0], [-1.0], [2.0], [0.5], [0.5], [2.0]], dtype=torch.float64)
    assert pc.pag_guidance(e, 2, 7.5, 3.0, False).flatten().tolist() == [13.0, 5.75]
    assert pc.pag_guidance(e[2:], 2, 7.5, 3.0, True).flatten().tolist() == [6.5, -4.0]


# ---------------------------------------------------------------------------------------------------- plan keys and launch lists
def test_plans_without_pag_are_what_they_were_and_pag_plans_hold_the_prefixes():
    from blobctrl_amd import _lib, pag
    eng = _engine()
    mid = pag.resolve_layers(eng.unet_cfg, "mid")
    ident = lambda P: [[(m["kind"], m["variant"], m["shape"], m["sid"]) for m in seg.meta] for seg in (P.prologue, P.step_active, P.step_inactive)]
    P0 = eng.plan_for(1, 8, 8, 7, TINY["ctx"], 3)
    key0 = list(eng._plans)[-1]
    assert key0 == (1, 8, 8, 7, TINY["ctx"], 3, False, False) and P0.pag == () and P0.pag_table is None and "pag_table" not in P0.rec.named
    P0b = eng.plan_for(1, 8, 8, 7, TINY["ctx"], 3, pag=())
    assert P0b is P0 and list(eng._plans) == [key0]
    kinds0 = [k for seg in ident(P0) for k, *_ in seg]
    assert "attention_identity" not in kinds0
    # ... and they are the listings the commit BEFORE this feature recorded (kind, variant, shape and stream of every launch of the three
    # segments, hashed there): 41 + 850 + 416 launches for the CFG plan, and for the single-pass plan of two requests
    digest = lambda P: hashlib.sha256(repr(ident(P)).encode()).hexdigest()[:16]
    assert [len(x) for x in ident(P0)] == [41, 850, 416] and digest(P0) == "0718783c90d90cee"
    assert digest(eng.plan_for(2, 8, 8, 7, TINY["ctx"], 3, single=True)) == "241b047b7124d1ee"
    P1 = eng.plan_for(1, 8, 8, 7, TINY["ctx"], 3, pag=mid)
    key1 = list(eng._plans)[-1]
    assert key1 == key0 + (("pag",) + mid,) and not any(isinstance(x, float) for x in key1[6:] + key1[-1])
    assert P1.ctx.shape[0] == 3 and P1.unet_in.shape[0] == 3 and P1.blob_in.shape[0] == 1 and P1.pag_table.shape == (3,)
    assert P1.rec.named["pag_table"] is P1.pag_table and not P1.split_cfg
    for seg in (P1.step_active, P1.step_inactive):
        kinds = [m["kind"] for m in seg.meta]
        assert kinds.count("attention_identity") == 1 and kinds[-1] == "cfg_step" and "dup_halves" not in kinds
        i = kinds.index("attention_identity")
        assert kinds[i - 1] == "attention" and seg.meta[i - 1]["shape"][0] == 2 and seg.meta[i]["shape"][1] == 1      # 2 images attend, 1 is perturbed
    # the guidance-free form: [cond | perturbed]; all 16 layers
    every = pag.resolve_layers(eng.unet_cfg, ["down", "mid", "up"])
    P2 = eng.plan_for(2, 8, 8, 7, TINY["ctx"], 3, single=True, pag=every)
    assert len(every) == 16 and P2.ctx.shape[0] == 4 and [m["kind"] for m in P2.step_active.meta].count("attention_identity") == 16
    assert list(eng._plans)[-1][-2:] == ("single", ("pag",) + every)
    # the plain plan recorded AFTER the PAG plans is the plan recorded before them
    eng2 = _engine()
    eng2.plan_for(1, 8, 8, 7, TINY["ctx"], 3, pag=mid)
    assert ident(eng2.plan_for(1, 8, 8, 7, TINY["ctx"], 3)) == ident(P0)
    # the op codes the PAG plan recorded are the new ones, and no old table knows them
    assert _lib.op_code("bc_attention_identity") == 60 and _lib.op_code("bc_pag_scheduler_step") == 61


def test_full_width_pag_plan_records_the_identity_behind_the_mid_attention():
    """SD-1.5 widths at a 32 x 32 latent (weights are zeros: a plan's launches do not depend on their values): a PAG plan with "mid" holds
    one bc_attention_identity per UNet forward, behind the mid block's attention, which runs on the two images in front."""
    from blobctrl_amd import pag, synth
    from blobctrl_amd.engine import TrunkConfig
    from blobctrl_amd.pipeline import BlobCtrlEngine
    boc = (320, 640, 1280, 1280)
    us = synth.trunk_param_shapes(5, boc, 2, 768, 4, blobnet=False)
    bs = synth.trunk_param_shapes(1029, boc, 2, None, None, blobnet=True)
    zeros = lambda sh: {k: torch.zeros(1).expand(*v) if len(v) else torch.zeros(()) for k, v in sh.items()}
    ucfg = TrunkConfig(in_channels=5)
    eng = BlobCtrlEngine(zeros(us), zeros(bs), ucfg, TrunkConfig(in_channels=1029, cross_attention_dim=None, out_channels=0, is_blobnet=True),
                         device="cpu", scheduler="ddim", compile_only=True, max_cached_plans=2)
    P = eng.plan_for(1, 32, 32, 77, 768, 2, pag=pag.resolve_layers(ucfg, "mid"))
    for seg in (P.step_active, P.step_inactive):
        meta = [m for m in seg.meta if m["sid"] == 0]
        kinds = [m["kind"] for m in meta]
        i = kinds.index("attention_identity")
        assert kinds.count("attention_identity") == 1 and meta[i]["shape"] == ("attention_identity", 1, 4 * 8, 1280)
        assert kinds[i - 1] == "attention" and meta[i - 1]["shape"] == (2, 8, 160, 32, 32) and "dup_halves" not in kinds


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_say_why():
    from blobctrl_amd import pag
    eng = _engine()
    mid = pag.resolve_layers(eng.unet_cfg, "mid")
    with pytest.raises(NotImplementedError, match="per-request schedules"):
        eng.plan_for(2, 8, 8, 7, TINY["ctx"], 3, per_request=True, requests=True, pag=mid)
    with pytest.raises(NotImplementedError, match="per-request schedules"):
        eng._pag_layers(3.0, 0.0, mid, listed=True)
    for kw in (dict(pag_scale=[3.0, 1.0]), dict(pag_scale=3.0, pag_adaptive_scale=[0.1, 0.2])):
        with pytest.raises(NotImplementedError, match="a list of per-request values"):
            eng.denoise(torch.zeros(2, 7, TINY["ctx"]), torch.zeros(1, 4, 8, 8), torch.zeros(1, 4, 8, 8), torch.zeros(1, 2, 8, 8),
                        torch.zeros(1, 1, TINY["feat"]), pag_applied_layers=mid, **kw)
    with pytest.raises(NotImplementedError, match="per-request schedules"):
        eng.denoise(torch.zeros(4, 7, TINY["ctx"]), torch.zeros(2, 4, 8, 8), torch.zeros(2, 4, 8, 8), torch.zeros(2, 2, 8, 8),
                    torch.zeros(2, 1, TINY["feat"]), num_inference_steps=[2, 3], pag_scale=3.0, pag_applied_layers=mid)
    with pytest.raises(ValueError, match="no self-attention block prefix"):
        eng._pag_layers(3.0, 0.0, ("mid",))
    with pytest.raises(NotImplementedError, match="in-process only"):
        eng.compile_plan("/nonexistent/x.bcplan", 1, 8, 8, 7, TINY["ctx"], 3, pag_scale=3.0, pag_applied_layers=mid)
    assert eng._pag_layers(0.0, 0.0, mid) == () and eng._pag_layers(3.0, 0.0, None) == () and eng._pag_layers(3.0, 0.0, ()) == ()
    assert not eng._plans                                                          # nothing was recorded on the way to a refusal


def test_pipeline_surface_has_the_reference_names_and_defaults():
    import inspect
    from blobctrl_amd.pipeline import BlobCtrlEngine, StableDiffusionBlobNetPipeline as Pipe
    sig = inspect.signature(Pipe.__call__).parameters
    assert sig["pag_scale"].default == 0.0 and sig["pag_adaptive_scale"].default == 0.0
    assert inspect.signature(Pipe.__init__).parameters["pag_applied_layers"].default == "mid"
    assert inspect.signature(Pipe.from_pretrained).parameters["pag_applied_layers"].default == "mid"
    d = inspect.signature(BlobCtrlEngine.denoise).parameters
    assert (d["pag_scale"].default, d["pag_adaptive_scale"].default, d["pag_applied_layers"].default) == (0.0, 0.0, None)
    p = Pipe.__new__(Pipe)
    p._pag_scale, p._pag_adaptive_scale = 0.0, 0.0
    p.set_pag_applied_layers("mid")
    assert p.pag_applied_layers == ["mid"] and not p.do_perturbed_attention_guidance and not p.do_pag_adaptive_scaling
    p._pag_scale = 3.0
    assert p.do_perturbed_attention_guidance and not p.do_pag_adaptive_scaling and p.pag_scale == 3.0
    p._pag_adaptive_scale = 0.01
    assert p.do_pag_adaptive_scaling and p.pag_adaptive_scale == 0.01
    p.set_pag_applied_layers(["down_blocks.1", "up_blocks.(1|2)"])
    assert p.pag_applied_layers == ["down_blocks.1", "up_blocks.(1|2)"]
    with pytest.raises(ValueError, match="Expected either a string or a list of string"):
        p.set_pag_applied_layers(7)
    p.set_pag_applied_layers([])
    assert not p.do_perturbed_attention_guidance


# ---------------------------------------------------------------------------------------------------- symbols and ops
def test_pag_symbols_resolve_and_their_ops_collide_with_no_table(tmp_path):
    import ctypes as C
    from blobctrl_amd import _lib
    lib = _lib.load()
    assert set(_lib.PAG_SIGNATURES) == set(_lib.PAG_OPS) == {"bc_attention_identity", "bc_pag_scheduler_step"}
    for name in _lib.PAG_SIGNATURES:
        assert getattr(lib, name) is not None and name not in _lib.EXPORTED_SYMBOLS
        assert not any(name in t for t in _lib._OP_TABLES + _lib._OP_TABLES_BEYOND + _lib._OP_TABLES_TINY_VAE)
    assert len(_lib.EXPORTED_SYMBOLS) == 92 and _lib._OP_TABLES_PAG == (_lib.PAG_OPS,)
    older = [c for t in _lib._OP_TABLES + _lib._OP_TABLES_BEYOND + _lib._OP_TABLES_TINY_VAE for c in t.values()] + [_lib.OP_SIGNAL, _lib.OP_WAIT]
    assert sorted(older) == [c for c in range(59) if c not in (54, 56)] and not set(older) & set(_lib.PAG_OPS.values())
    assert _lib.PAG_OPS == {"bc_attention_identity": 60, "bc_pag_scheduler_step": 61}
    assert _lib.op_signature("bc_attention_identity") == "ppiiiiii" and _lib.op_signature("bc_pag_scheduler_step") == "ppppppiiipiiipi"
    # the plan runtime takes both with their argument counts, refuses one fewer, and 59 (BC_OP_TINY_VAE_END) and 62 (BC_OP_PAG_END) are no ops
    plan = C.c_void_p()
    assert lib.bc_plan_create(C.byref(plan)) == 0
    try:
        seg = lib.bc_plan_segment(plan, b"s")
        words = (C.c_uint64 * 16)()
        assert lib.bc_plan_add_op(plan, seg, 0, 60, words, 8) == 0 and lib.bc_plan_add_op(plan, seg, 0, 61, words, 15) == 1
        assert lib.bc_plan_add_op(plan, seg, 0, 60, words, 7) < 0 and b"op 60 takes 8" in lib.bc_last_error()
        assert lib.bc_plan_add_op(plan, seg, 0, 61, words, 14) < 0
        assert lib.bc_plan_add_op(plan, seg, 0, 59, words, 8) < 0 and lib.bc_plan_add_op(plan, seg, 0, 62, words, 8) < 0
        buf = (_lib.BcPlanBuffer * 1)()
        buf[0].name, buf[0].address, buf[0].bytes = b"x", 0x1000, 16
        path = str(tmp_path / "pag.bcplan")
        assert lib.bc_plan_save(plan, path.encode(), buf, 1) != 0 and b"in-process only" in lib.bc_last_error() and not os.path.exists(path)
    finally:
        lib.bc_plan_destroy(plan)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Argument checks come before the launch, so they run without a device."""
    from blobctrl_amd import _lib
    lib = _lib.load()
    a = 1 << 20                                                                    # (an aligned address that is never dereferenced)
    bad = [(a, a, 2, 3, 64, 16, 64, 16), (a, a, 2, 1, 64, 12, 64, 16), (a, a, 2, 1, 72, 16, 72 - 8, 16), (a, a, 2, 1, 64, 16, 64, 8),
           (a + 2, a, 2, 1, 64, 16, 64, 16), (None, a, 2, 1, 64, 16, 64, 16), (a, a, 2, 1, 64, 16, 68, 16)]
    for args in bad:
        assert lib.bc_attention_identity(*args, None) == 1 and b"bc_attention_identity" in lib.bc_last_error(), args
    assert lib.bc_pag_scheduler_step(a, a, a, a, a, None, 1, 2, 2, None, 3, 0, 0, a, 1, None) == 1 and b"bc_pag_scheduler_step" in lib.bc_last_error()
    assert lib.bc_pag_scheduler_step(a, a, a, a, a, a, 1, 2, 2, None, 0, 0, 0, a, 1, None) == 1
