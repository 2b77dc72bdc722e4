"""`Recorder.gemm` asks the library how a BcGemm launches (bc_gemm_resolve) instead of working it out again: what it records did not change
with that.  tests/golden/gemm_records_before_resolve.json holds, per source of tests/gemm_records_common.py, the hash of every launch's
`meta`, every BcGemm record and the slab reserved per stream as the commit BEFORE wrote them; here they are recorded again (CPU,
compile-only) and compared, and bc_gemm_resolve is asked about every recorded struct: it names the split count, the reducer and the
kernel the `meta` names.  (`python tools/make_plan_fixture.py --gemm-records-text NAME` prints a source's text for a diff.)"""
import ctypes as C
import json
import os

import pytest

from blobctrl_amd import _lib
from tests import gemm_records_common as gr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_records_before_resolve.json")


@pytest.fixture(scope="module")
def recorded():
    """{source: Capture}, every source recorded once for the tests below."""
    return {name: record() for name, record in gr.sources()}


def test_the_sources_are_the_frozen_ones(recorded):
    frozen = json.load(open(GOLD))
    assert sorted(frozen) == sorted(recorded) and len(frozen) == 81 + 6 + 2 + 247
    assert sum(frozen[n]["gemms"] for n in frozen if n.startswith("planner/")) == 316


def test_records_equal_the_ones_frozen_before_the_library_resolved_them(recorded):
    frozen = json.load(open(GOLD))
    differ = [name for name, cap in recorded.items() if cap.entry() != frozen[name]]
    assert not differ, f"{len(differ)} of {len(recorded)} sources record differently: {differ[:8]}"


def test_the_library_resolves_every_record_to_what_its_meta_says(recorded):
    lib, n = _lib.load(), 0
    for name, cap in recorded.items():
        for g, m in zip(cap.gemms, cap.gemm_launches()):
            q = _lib.BcGemm()
            C.memmove(C.byref(q), C.byref(g), C.sizeof(g))
            q.slab = None                                      # (what a record holds: the slab is bound at replay)
            info = _lib.BcGemmInfo()
            assert lib.bc_gemm_resolve(C.byref(q), C.byref(info)) == 0, (name, m, lib.bc_last_error())
            assert info.splitk == m["shape"][-1], (name, m, info.splitk)
            assert (info.splitk > 1) == m["variant"].endswith("+splitk_reduce"), (name, m)
            assert info.kernel.decode() == m["rocprof"], (name, m, info.kernel)
            assert info.slab_elems == (info.splitk * g.M * g.N if info.splitk > 1 else 0)
            n += 1
    assert n == sum(len(c.gemms) for c in recorded.values()) > 3900


OVERRIDE_SCRIPT = """
import torch
from blobctrl_amd.launch import Recorder
from tests import gemm_views_common as gv
from tests.gemm_records_common import record_view
rec = Recorder(torch.device("cpu"))
for mode in ("dense", "splitk3_R"):
    record_view(rec, gv.build(gv.fast_case(2, mode), "vec", torch.device("cpu")))
    m = rec.seg.meta[-1]
    print(m["variant"], "|", m["rocprof"], "|", m["shape"][-1])
"""


@pytest.mark.parametrize("env,want", [
    # (the generic kernel at N = 200: a 128-wide tile would pad N by 28 %, over bc_gemm_plan's 10 %, so the 256 x 64 tile)
    (dict(BC_GEMM_GENERIC="1"), ["gemm_kernel<256x64_s2,dense> | gemm_kernel<256, 64, 4, 1> | 1",
                                 "gemm_kernel<256x64_s2,dense>+splitk_reduce | gemm_kernel<256, 64, 4, 1> | 3"]),
    (dict(BC_GEMM_TILE="7"), ["gemm_fast_kernel<64x64,dense> | gemm_fast_kernel<64, 64, 2, 2, 4, false, false> | 1",
                              "gemm_fast_kernel<64x64,dense>+splitk_reduce | gemm_fast_kernel<64, 64, 2, 2, 4, false, false> | 3"])],
    ids=["BC_GEMM_GENERIC", "BC_GEMM_TILE"])
def test_the_recorder_follows_the_librarys_environment_overrides(env, want):
    """BC_GEMM_GENERIC / BC_GEMM_TILE are read by the library alone (once per process: hence a child process); a record made under one names
    the kernel and the tile the library resolves - here for problems recorded with tile 128x128_s3 asked for."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", OVERRIDE_SCRIPT], cwd=repo, env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines() == want
