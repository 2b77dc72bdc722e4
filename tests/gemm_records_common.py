"""What `Recorder.gemm` records, frozen (tests/test_gemm_records_cpu.py, tools/make_plan_fixture.py --gemm-records): for a list of sources -
the planner cases, full-width SD-1.5 plans, the tiny-net plans, the view problems of tests/gemm_views_common.py - every launch's `meta`,
every `BcGemm` handed to bc_plan_add_gemm and the split-K slab reserved per stream, as one canonical text per source.  Everything here
records on the CPU; nothing is launched."""
import contextlib
import ctypes as C
import hashlib
import json
import os

import torch

from blobctrl_amd import _lib

CPU = torch.device("cpu")
POINTERS = {name for name, ct in _lib.BcGemm._fields_ if ct is C.c_void_p}
FULL_PLANS = [(1, 64, False), (2, 64, False), (4, 64, False), (8, 64, False), (1, 96, False), (1, 64, True)]       # (B, h = w, freeu)


class Capture:
    """Recorders created and BcGemm structs handed to bc_plan_add_gemm, in order, while `capture()` is open."""

    def __init__(self):
        self.recorders, self.gemms, self.where = [], [], []

    def launches(self):
        return [m for r in self.recorders for s in r.segments for m in s.meta]

    def gemm_launches(self):
        """The `meta` of every bc_gemm record, in the order of `gemms`."""
        return [next(s for s in rec.segments if s.id == seg).meta[idx] for rec, seg, idx in self.where]

    def text(self):
        lines = ["L " + json.dumps(m, sort_keys=True, default=str) for m in self.launches()]
        for g in self.gemms:
            fields = []
            for name, _ in _lib.BcGemm._fields_:
                v = getattr(g, name)
                fields.append(f"{name}=" + (("null" if not v else f"ptr%16={v % 16}") if name in POINTERS else repr(v)))
            lines.append("G " + " ".join(fields))
        for i, r in enumerate(self.recorders):
            lines += [f"S recorder {i} stream {sid}: {n}" for sid, n in sorted(r._slab_elems.items())]
        return "\n".join(lines) + "\n"

    def entry(self):
        return dict(launches=len(self.launches()), gemms=len(self.gemms), sha256=hashlib.sha256(self.text().encode()).hexdigest())


@contextlib.contextmanager
def capture(plan_opts=None):
    """Record under BC_PLAN = `plan_opts` (none: the defaults) with every new Recorder and every bc_plan_add_gemm struct kept."""
    from blobctrl_amd import launch
    cap, lib = Capture(), _lib.load()
    add, init = lib.bc_plan_add_gemm, launch.Recorder.__init__

    def add_gemm(plan, seg, sid, ref):
        g = _lib.BcGemm()
        C.memmove(C.byref(g), C.byref(ref._obj), C.sizeof(g))
        idx = add(plan, seg, sid, ref)
        cap.gemms.append(g)
        cap.where.append((next(r for r in cap.recorders if r.plan is plan), seg, idx))
        return idx

    def new_recorder(self, *a, **k):
        init(self, *a, **k)
        cap.recorders.append(self)

    saved = os.environ.pop("BC_PLAN", None)
    if plan_opts:
        os.environ["BC_PLAN"] = ",".join(f"{k}={int(v)}" for k, v in plan_opts.items())
    lib.bc_plan_add_gemm, launch.Recorder.__init__ = add_gemm, new_recorder
    try:
        yield cap
    finally:
        lib.bc_plan_add_gemm, launch.Recorder.__init__ = add, init
        os.environ.pop("BC_PLAN", None)
        if saved is not None:
            os.environ["BC_PLAN"] = saved


# ---------------------------------------------------------------------------------------------------- sources
def view_cases(front_end=False):
    """The cases of the view tables that were frozen (tests/golden/gemm_records_before_resolve.json); front_end: the front ends' launch forms
    added since (Case.front_end) as well."""
    from tests import gemm_views_common as gv
    cases = gv.generic_cases() + [gv.fast_case(cfg, mode) for cfg in range(1, 8) for mode in gv.FAST_MODES]
    cases += gv.gw_cases() + gv.g256_cases() + gv.halo_cases("halo") + gv.halo_cases("wreg")
    return [c for c in cases if front_end or not c.front_end]


def view_problems(front_end=False):
    """Every (case, flavour) problem of the view tables, built on the CPU."""
    from tests import gemm_views_common as gv
    for case in view_cases(front_end):
        for flavour in gv.FLAVOURS:
            yield gv.build(case, flavour, CPU)


def record_view(rec, prob):
    """tests/test_gemm_views_gpu.py::launch without the run: the problem's one Recorder.gemm on `rec`."""
    from blobctrl_amd.launch import encode_gn_tot
    kw = dict(prob.kw)
    if rec.seg is None:
        rec.begin("views")
    if prob.gn_in:
        gi, srcs = prob.gn_in, []
        for name, Cc, sums in gi["srcs"]:
            x, tot = prob.views[name].t, encode_gn_tot(sums)
            rec.tots[x.data_ptr()] = tot
            rec.tots_per_channel.add(id(tot))
            rec.keep.append(tot)
            srcs.append((x, Cc))
        x2, C2 = srcs[1] if len(srcs) > 1 else (None, 0)
        kw["a_gn"] = dict(x1=srcs[0][0], C1=srcs[0][1], x2=x2, C2=C2, B=gi["B"], HW=gi["HW"], G=gi["G"], eps=gi["eps"], gamma=gi["gamma"],
                          beta=gi["beta"])
    rec.gemm(**kw)


def _full_engine():
    """A compile-only engine at full SD-1.5 widths; zero weights (a plan's launches do not depend on their values)."""
    from blobctrl_amd import synth
    from blobctrl_amd.engine import TrunkConfig
    from blobctrl_amd.pipeline import BlobCtrlEngine
    boc = (320, 640, 1280, 1280)
    us = synth.trunk_param_shapes(5, boc, 2, 768, 4, blobnet=False)
    bs = synth.trunk_param_shapes(1029, boc, 2, None, None, blobnet=True)
    zeros = lambda sh: {k: torch.zeros(1).expand(*v) if len(v) else torch.zeros(()) for k, v in sh.items()}
    return BlobCtrlEngine(zeros(us), zeros(bs), TrunkConfig(in_channels=5),
                          TrunkConfig(in_channels=1029, cross_attention_dim=None, out_channels=0, is_blobnet=True), device="cpu",
                          scheduler="ddim", compile_only=True, max_cached_plans=1)


def _tiny_engine():
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from tests.common import tiny_weights
    from tests.gpu_common import tiny_trunk_configs
    usd, bsd = tiny_weights()
    ucfg, bcfg = tiny_trunk_configs()
    return BlobCtrlEngine(usd, bsd, ucfg, bcfg, device="cpu", scheduler="unipc", compile_only=True, max_cached_plans=1)


def sources():
    """(name, record) pairs: record() opens its own capture and returns it."""
    from tests import planner_cases as pc
    from tests.common import TINY
    out = []

    def planner(case):
        def run():
            with capture(case.opts) as cap:
                rec, _, _ = pc.record(case, CPU)
            rec.close()
            return cap
        return run

    def plan(make, state, *args, **kw):
        def run():
            if "eng" not in state:
                state["eng"] = make()
            with capture() as cap:
                state["eng"].plan_for(*args, **kw)
            return cap
        return run

    def view(prob):
        def run():
            from blobctrl_amd.launch import Recorder
            with capture() as cap:
                rec = Recorder(CPU)
                record_view(rec, prob)
            rec.close()
            return cap
        return run

    out += [(f"planner/{c.id}", planner(c)) for c in pc.CASES]
    full, tiny = {}, {}
    out += [(f"full/B{B}-{hw}x{hw}" + ("-freeu" if fu else ""), plan(_full_engine, full, B, hw, hw, 77, 768, 2, freeu=fu)) for B, hw, fu in FULL_PLANS]
    out += [(f"tiny/B{B}", plan(_tiny_engine, tiny, B, 8, 8, 7, TINY["ctx"], 6)) for B in (1, 3)]
    out += [(f"views/{p.name}", view(p)) for p in view_problems() if not p.refused]
    return out
