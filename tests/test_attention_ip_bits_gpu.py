"""The output bits of the four IP-Adapter attention kernels (csrc/attention_ip.hip, csrc/attention_ip_masked.hip), pinned: one launch per
case by name at w = 0.35 (tests/attention_ip_bits_common.py lists the cases), and the sha256 of the whole parent buffer of O as int16,
fences included, against tests/golden/attention_ip_bits.json.

The JSON was written by `python -m tests.test_attention_ip_bits_gpu` (write_golden below), run once on an MI355X against the library
built from the commit in front of the one that moved the kernels' shared parts into csrc/bc_attention_ip.h: the kernels as they were
written twice.  It holds, per case, that digest and the digest of the case's CPU-made inputs (tests/test_attention_ip_bits_cpu.py
asserts those without a device, and this test asserts them first: drift of the inputs is not drift of a kernel).  A kernel change that is
meant to leave the numerics alone must match every digest; a mismatch is fixed in the kernel, not here."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

from blobctrl_amd import _lib  # noqa: E402
from tests import attention_ip_bits_common as bc  # noqa: E402

DEV = torch.device("cuda:0")


def _ptr(x):
    return x.data_ptr() if torch.is_tensor(x) else x


def run_case(kind, path, params):
    """(digest of the CPU inputs, digest of O's parent buffer after one launch of the named path)."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    lib = _lib.load()
    with bc.rows_as(bc.rows_of(kind, params)):
        prob = bc.problem(DEV, kind, params)
        prob.assert_inside()
        entry = lib.bc_attention_ip_with if kind == "plain" else lib.bc_attention_ip_masked_with
        rc = entry(path, *[_ptr(a) for a in prob.args()], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _lib.check(rc, f"{kind} path {path}")
    return bc.digest(*prob.cpu[:5]), bc.digest(prob.o.parent.view(torch.int16).cpu())


@pytest.fixture(scope="module")
def golden():
    return bc.load_golden()


@pytest.mark.parametrize("name,kind,path,params", bc.cases(), ids=[c[0].replace(" ", "_") for c in bc.cases()])
def test_output_bits_are_the_pinned_ones(golden, name, kind, path, params):
    inputs, out = run_case(kind, path, params)
    assert inputs == golden[name]["inputs"], f"{name}: the CPU-made inputs are not the ones the digest was taken on"
    assert out == golden[name]["o"], f"{name}: the bits of O (fences included) differ from the pinned ones"


def test_every_case_is_pinned(golden):
    assert sorted(golden) == sorted(c[0] for c in bc.cases())


def write_golden():
    out = {}
    for name, kind, path, params in bc.cases():
        inputs, o = run_case(kind, path, params)
        out[name] = {"inputs": inputs, "o": o}
        print(name, o[:16], flush=True)
    with open(bc.GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cases -> {bc.GOLDEN}")


if __name__ == "__main__":
    write_golden()
