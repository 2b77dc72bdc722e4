"""The edit plan on the host: what `PlanSpec` says of a plan (key, refusals, derived values, step call) and the plans the engine records
from it.  The digests below were written by the commit BEFORE `blobctrl_amd/edit_plan.py` existed, with this file's own helpers: every
buffer (index, name, bytes) and every launch (op, stream, arguments, pointers as buffer + offset) of the compiled forms, and for the forms
that are recorded in-process only (IP-Adapter, PAG) the listing, the named buffers and the key.  A plan that records another launch,
argument or buffer than that commit did changes its digest."""
import hashlib
import inspect
import os

import pytest
import torch

from tests.common import TINY, build_plan_dump

ARGS = (8, 8, 7, TINY["ctx"])                                      # h, w, T, ctx_dim of every plan here


@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    return build_plan_dump(tmp_path_factory.mktemp("dump"))


def _engine(kind="ddim"):
    from blobctrl_amd import schedulers
    from tests.test_pag_cpu import _engine as make
    eng = make()
    sd = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000)
    s = {"heun": lambda: schedulers.HeunDiscreteScheduler(**sd), "dpm3": lambda: schedulers.DPMSolverMultistepScheduler(solver_order=3),
         "ddim": lambda: None}[kind]()
    if s is not None:
        eng.set_scheduler(s.kind, s.table_params())
    return eng


# ---------------------------------------------------------------------------------------------------- compiled forms
# name: (scheduler, B, steps, keywords of compile_plan, BC_SPLIT_CFG)
COMPILED = {
    "plain": ("ddim", 2, 3, {}, False),
    "eta": ("ddim", 2, 3, dict(eta=1.0), False),
    "single": ("ddim", 2, 3, dict(guidance_scale=1.0, single_pass=True), False),
    "freeu": ("ddim", 1, 3, dict(freeu=(0.9, 0.2, 1.2, 1.4)), False),
    "requests": ("ddim", 3, [4, 2, 3], dict(guidance_scale=[7.5, 1.0, 3.0]), False),
    "heun": ("heun", 1, 3, {}, False),
    "dpm3": ("dpm3", 1, 6, {}, False),                              # (a third-order row needs more than four steps)
    "window": ("ddim", 1, 4, dict(blobnet_control_guidance_end=0.5), False),
    "split_cfg": ("ddim", 1, 3, {}, True),
}
COMPILED_DIGESTS = {
    "plain": "9855814ce96eb20ddb70f51433b69326fbc18b75684747333a6e24e4b83b970a",
    "eta": "347c5d5c7194aee114508a48b001e24152d39c89abdfbfd8d946400413825d4e",
    "single": "a9464f386226319e7588d876954d6f647a9d6ac4ac54dd0b2cec470b58ff136b",
    "freeu": "671938baca055c87d92da58a597ebf2d801a31a5365ffaca920b096d4fbe4bc0",
    "requests": "ffad651f5b07fa61b66078d74671a2cc44e202019e83b262916bc58f9df7c249",
    "heun": "c351a6f32b8fc9db13f6e220fcee42685f87ddb858c8930a31dff29be85f7e87",
    "dpm3": "84db3dbdc2b806e4a15e32ee426e856fed733fac4706fabcae0296bc73a126a0",
    "window": "4aea784e2ac83dabab223d872578601c39d17c64d7a2ea84398b4f330d7be522",
    "split_cfg": "20b9ec63d73217311a51564ec743fbf15610736ab0efea1b0c122222b2e9bf0c",
}
# what tells the forms apart, checked on the plan itself so that a digest cannot be the digest of another form
COMPILED_FORMS = {
    "plain": dict(), "eta": dict(stochastic=True), "single": dict(single=True), "freeu": dict(freeu=True), "requests": dict(requests=True),
    "heun": dict(scaled=True), "dpm3": dict(third_order=True), "window": dict(), "split_cfg": dict(split_cfg=True),
}


@pytest.mark.parametrize("name", sorted(COMPILED))
def test_compiled_plan_is_the_plan_the_parent_commit_compiled(name, plan_dump, tmp_path, monkeypatch):
    kind, B, steps, kw, split = COMPILED[name]
    if split:
        monkeypatch.setenv("BC_SPLIT_CFG", "1")
    eng = _engine(kind)
    path = str(tmp_path / f"{name}.bcplan")
    seq = eng.compile_plan(path, B, *ARGS, steps, **kw)
    P = next(reversed(eng._plans.values()))
    form = dict(stochastic=False, third_order=False, scaled=False, single=False, requests=False, split_cfg=False, freeu=False)
    form.update(COMPILED_FORMS[name])
    got = dict(stochastic=P.stochastic, third_order=P.third_order, scaled=P.scaled, single=P.single, requests=P.requests,
               split_cfg=P.split_cfg, freeu=P.freeu is not None)
    assert got == form, name
    if name == "window":
        assert seq == ["step_active", "step_active", "step_inactive", "step_inactive"]
    bufs, segs = plan_dump(path)
    digest = hashlib.sha256(repr((sorted(bufs.items()), sorted(segs.items()), seq)).encode()).hexdigest()
    print(f"compiled {name}: {len(bufs)} buffers, {[len(v) for _, v in sorted(segs.items())]} launches, sha256 {digest}")
    assert digest == COMPILED_DIGESTS[name], name


def test_compiled_digests_tell_the_forms_apart():
    assert len(set(COMPILED_DIGESTS.values())) == len(COMPILED_DIGESTS) == len(COMPILED)


# ---------------------------------------------------------------------------------------------------- in-process-only forms
def _ip_engine(name):
    from tests import clip_vision_common as cv
    from tests.test_ip_adapter_cpu import _engine as base
    from tests.test_ip_plus_cpu import _engine as plus
    return plus([cv.tiny_plus_adapter("q16")]) if name == "ip_plus" else base(1 if name == "ip_one" else 2)


def _in_process(name):
    """(engine, plan) of an in-process-only form."""
    from blobctrl_amd import pag
    from tests import clip_vision_common as cv
    if name.startswith("ip_"):
        eng = _ip_engine(name)
        kw = {"ip_one": dict(ip=(1,)), "ip_two": dict(ip=(2, 1)), "ip_two_masked": dict(ip=(2, 1), ip_masked=True),
              "ip_plus": dict(ip=((1, cv.PLUS_SEQ),))}[name]
        return eng, eng.plan_for(1, *ARGS, 3, **kw)
    eng = _engine()
    if name == "pag_mid":
        return eng, eng.plan_for(1, *ARGS, 3, pag=pag.resolve_layers(eng.unet_cfg, "mid"))
    every = pag.resolve_layers(eng.unet_cfg, ["down", "mid", "up"])
    assert name == "pag_all_single" and len(every) == 16
    return eng, eng.plan_for(2, *ARGS, 3, single=True, pag=every)


IN_PROCESS_DIGESTS = {
    "ip_one": "1bfc6ef7e711e02b73bd92a484d99d64c38bae27663fd99f3c2d7f18a9152d33",
    "ip_two": "c4ffc7fb5adbf7196f350b1909827102ef5d674e68187acf4f5479ec5aef6cda",
    "ip_two_masked": "b1840153aa8997ef1bba32637b5bf9bca81868452b8d85750f03bd10e110681c",
    "ip_plus": "a52ab6cdb2905b985467bf831105739a719937fefecaf42a8c3faec58ac20666",
    "pag_mid": "1b605fc2798aab4b9b313d045dacc5040b568fd7d82df5550ceabfb2fb45de4c",
    "pag_all_single": "1b643767d9271948a8f13cb0ab6923be91f7d18c1253352b6767743032fc0f18",
}


@pytest.mark.parametrize("name", sorted(IN_PROCESS_DIGESTS))
def test_in_process_plan_is_the_plan_the_parent_commit_recorded(name):
    eng, P = _in_process(name)
    key = list(eng._plans)[-1]
    listing = [[(m["kind"], m["variant"], m["shape"], m["sid"]) for m in seg.meta] for seg in (P.prologue, P.step_active, P.step_inactive)]
    named = sorted((n, tuple(t.shape), str(t.dtype)) for n, t in P.rec.named.items())
    digest = hashlib.sha256(repr((listing, named, key)).encode()).hexdigest()
    print(f"in-process {name}: {[len(x) for x in listing]} launches, {len(named)} named buffers, key {key}, sha256 {digest}")
    assert digest == IN_PROCESS_DIGESTS[name], name


def test_in_process_digests_tell_the_forms_apart():
    assert len(set(IN_PROCESS_DIGESTS.values())) == len(IN_PROCESS_DIGESTS)


# ---------------------------------------------------------------------------------------------------- the spec
def _adapters(n):
    """Stand-ins for loaded adapters, as far as a key reads them (weights.ip_adapter_tokens / ip_adapter_embed_dim)."""
    from tests.test_ip_adapter_cpu import _engine as base
    return base(n).ip_adapters


def test_spec_keys_are_the_tuples_the_plans_are_cached_under():
    from blobctrl_amd.edit_plan import PlanSpec
    from tests import clip_vision_common as cv
    from tests import ip_adapter_common as ipc
    ctx = TINY["ctx"]
    base = (1, 8, 8, 7, ctx, 3, False, False)
    assert PlanSpec(1, 8, 8, 7, ctx, 3).key(()) == base
    assert PlanSpec(1, 8, 8, 7, ctx, 3, pag=None).key(()) == base and PlanSpec(1, 8, 8, 7, ctx, 3, pag=[]).pag == ()
    mid = ("mid_block.attentions.0.",)
    assert PlanSpec(1, 8, 8, 7, ctx, 3, pag=list(mid)).key(()) == base + (("pag",) + mid,)
    every = tuple(f"p{i}." for i in range(16))
    assert PlanSpec(2, 8, 8, 7, ctx, 3, single=True, pag=every).key(())[-2:] == ("single", ("pag",) + every)
    # every switch, in the order the key has always had; the booleans are normalised (1 is True)
    full = PlanSpec(3, 8, 8, 7, ctx, 4, per_request=True, stochastic=1, scaled=1, single=1, freeu=1, requests=1)
    assert full.key(()) == (3, 8, 8, 7, ctx, 4, True, True, "scaled", "single", "freeu", "requests")
    assert PlanSpec(1, 8, 8, 7, ctx, 6, third_order=True).key(()) == (1, 8, 8, 7, ctx, 6, False, False, "step3")
    assert all(type(getattr(full, f)) is bool for f in ("per_request", "stochastic", "third_order", "scaled", "single", "freeu", "requests", "ip_masked"))
    # adapters: count, (tokens, embedding width) each; masks add their own entry with the images per adapter
    two = _adapters(2)
    assert PlanSpec(1, 8, 8, 7, ctx, 3, ip=(1,)).key(two[:1]) == base + (("ip", 1, (4, ipc.IP_EMBED_DIM)),)
    assert PlanSpec(1, 8, 8, 7, ctx, 3, ip=(2, 1)).key(two) == base + (("ip", 2, (8, ipc.IP_EMBED_DIM), (4, ipc.IP_EMBED_DIM)),)
    masked = PlanSpec(1, 8, 8, 7, ctx, 3, ip=(2, 1), ip_masked=True).key(two)
    assert masked == base + (("ip", 2, (8, ipc.IP_EMBED_DIM), (4, ipc.IP_EMBED_DIM)), ("ip", "masked", 2, 1))
    assert PlanSpec(1, 8, 8, 7, ctx, 3, ip_masked=True).key(()) == base                # (masks without an adapter: the plain plan)
    plus = _ip_engine("ip_plus").ip_adapters
    assert PlanSpec(1, 8, 8, 7, ctx, 3, ip=((2, cv.PLUS_SEQ),)).key(plus)[-1] == ("ip", 1, (32, cv.PLUS_EMBED, cv.PLUS_SEQ))
    assert PlanSpec(1, 8, 8, 7, ctx, 3, ip=((2, cv.PLUS_SEQ),), ip_masked=True).key(plus)[-1] == ("ip", "masked", 2)


def test_spec_derived_values_and_step_call():
    from blobctrl_amd.edit_plan import PlanSpec
    S = lambda B=2, **kw: PlanSpec(B, 8, 8, 7, TINY["ctx"], 3, **kw)
    assert (S().Bi, S().Bu, S().cfg_pairs) == (1, 4, True)
    assert (S(per_request=True).Bi, S(single=True).Bu, S(single=True).cfg_pairs) == (2, 2, False)
    assert (S(pag=("a.",)).Bu, S(single=True, pag=("a.",)).Bu, S(pag=("a.",)).cfg_pairs) == (6, 4, False)
    assert [S(**kw).assemble_suffix for kw in ({}, dict(scaled=True), dict(scaled=True, per_request=True, requests=True),
                                               dict(per_request=True, requests=True))] == ["", "_scaled", "_requests", ""]
    # the precedence of the step entry points: PAG, requests, single, noise, third order, plain
    names = [S(**kw).step_call()[0] for kw in (dict(pag=("a.",), single=True, stochastic=True), dict(per_request=True, requests=True, single=True),
                                              dict(single=True, stochastic=True), dict(stochastic=True), dict(third_order=True), {})]
    assert names == ["bc_pag_scheduler_step", "bc_scheduler_step_requests", "bc_scheduler_step_single", "bc_cfg_scheduler_step_noise",
                     "bc_cfg_scheduler_step3", "bc_cfg_scheduler_step"]


def test_spec_refusals_are_the_three_the_planner_had():
    from blobctrl_amd.edit_plan import PlanSpec
    S = lambda **kw: PlanSpec(2, 8, 8, 7, TINY["ctx"], 3, **kw)
    with pytest.raises(ValueError, match=r"per-request schedules need a request batch \(per_request\)"):
        S(requests=True).validate()
    with pytest.raises(NotImplementedError, match="perturbed-attention guidance with per-request schedules: bc_pag_scheduler_step reads ONE coefficient "
                                                  "table and ONE pag_table; run the requests with shared steps, guidance scale, window and eta"):
        S(per_request=True, requests=True, pag=("mid_block.attentions.0.",)).validate()
    with pytest.raises(NotImplementedError, match=r"a third-order step has no noise term \(the reference's third-order update has no SDE branch\)"):
        S(stochastic=True, third_order=True).validate()
    S().validate()
    S(per_request=True, requests=True, stochastic=True).validate()
    eng = _engine()
    for kw in (dict(requests=True), dict(stochastic=True, third_order=True)):
        with pytest.raises((ValueError, NotImplementedError)):
            eng.plan_for(2, *ARGS, 3, **kw)
    assert not eng._plans and eng.cache_stats["plans_recorded"] == 0


def test_plan_for_keeps_its_signature_and_an_empty_pag_is_the_plain_plan():
    from blobctrl_amd.edit_plan import EditPlan, PlanSpec
    from blobctrl_amd.pipeline import BlobCtrlEngine
    assert list(inspect.signature(BlobCtrlEngine.plan_for).parameters) == ["self", "B", "h", "w", "T", "ctx_dim", "nsteps", "per_request", "stochastic",
                                                                          "third_order", "scaled", "single", "freeu", "requests", "ip", "ip_masked", "pag"]
    eng = _engine()
    P = eng.plan_for(1, *ARGS, 3)
    assert eng.plan_for(1, *ARGS, 3, pag=()) is P and eng._plan(PlanSpec(1, *ARGS, 3)) is P
    assert eng.cache_stats["plans_recorded"] == 1 and eng.cache_stats["plan_hits"] == 2 and list(eng._plans) == [(1,) + ARGS + (3, False, False)]
    # the plan declares what no form of it owns, and reads its switches from the spec it carries
    assert isinstance(P, EditPlan) and P.spec == PlanSpec(1, *ARGS, 3)
    for name in ("pag_table", "freeu", "variance_noise", "t_rows_unet", "t_rows_blob", "timestep_cond", "eps_all"):
        assert getattr(P, name) is None, name
    assert P.t_table is not None and (P.single, P.stochastic, P.third_order, P.scaled, P.requests, P.Bi, P.pag) == (False,) * 5 + (1, ())
    R = eng.plan_for(2, *ARGS, 3, per_request=True, requests=True)
    assert R.t_table is None and R.t_rows_unet.shape == (3, 4) and R.t_rows_blob.shape == (3, 2) and R.requests and R.Bi == 2


# ---------------------------------------------------------------------------------------------------- what the planner no longer holds
def test_dead_switches_and_anonymous_plans_are_gone():
    import blobctrl_amd
    root = os.path.dirname(blobctrl_amd.__file__)
    text = {f: open(os.path.join(root, f)).read() for f in ("pipeline.py", "edit_plan.py", "engine.py")}
    for word in ("temb_per_step", "no_im2col", 'type("Plan"'):
        assert word not in text["pipeline.py"] and word not in text["edit_plan.py"], word
    for word in ('getattr(self, "tproj_table"', 'getattr(self, "ctx_kvs"', 'getattr(self, "ctx_folded"', 'getattr(self, "w8_img"', 'getattr(unet_a',
                 'getattr(P, "pag_table"'):
        assert not any(word in t for t in text.values()), word
    # the state the forwards of a plan share is declared by the class that reads it
    from blobctrl_amd.engine import TrunkPlan
    plan = TrunkPlan(None, None, blobctrl_amd.engine.TrunkConfig(in_channels=5), 1, 8, 16)
    assert (plan.ctx_kv, plan.ctx_kvs, plan.ctx_folded, plan.ip_kv, plan.tproj, plan.tproj_table) == ({}, {}, {}, {}, None, ())
    assert (plan.w8_img, plan.res_events, plan.res_bmod) == (None, None, 1)
