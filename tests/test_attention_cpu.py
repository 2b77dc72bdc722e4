"""Which attention build a shape runs (bc_attention_build: host arithmetic, no device), over the loop's real launches, and the power of the
designed inputs of tests/attention_common.py on a small shape (the GPU tests assert it at every shape they use)."""
import pytest

from blobctrl_amd import _lib
from tests import attention_common as ac


@pytest.fixture(autouse=True)
def default_builds(monkeypatch):
    monkeypatch.delenv("BC_ATTN_NO8", raising=False)


def test_the_loops_attention_launches_select_the_expected_builds():
    lib = _lib.load()
    for shape, build in ac.LOOP_SHAPES:
        assert lib.bc_attention_build(*shape) == build, (shape, build)


def test_build_thresholds_and_unsupported_head_dims(monkeypatch):
    b = _lib.load().bc_attention_build
    # d = 80: the 8-wave form needs whole 256-query workgroups and a long key loop
    assert b(80, 1, 8, 2048, 2048, 0) == 81 and b(80, 1, 8, 2047, 2048, 0) == 41 and b(80, 1, 8, 2048, 1023, 0) == 41
    assert b(80, 1, 2, 512, 1024, 0) == 81 and b(80, 1, 2, 511, 1024, 0) == 41
    # d = 40: 256 workgroups of 256 queries -> 84; below that, or under BC_ATTN_NO8, the 4-wave forms (128-VGPR from 1024 workgroups)
    assert b(40, 4, 16, 1000, 1090, 0) == 84 and b(40, 4, 16, 768, 1090, 0) == 41 and b(40, 4, 16, 1000, 1023, 0) == 41
    assert b(40, 1, 8, 8192, 8192, 1) == 41                              # causal: always the default build
    for d in (8, 16, 32):
        assert b(d, 8, 16, 997, 1030, 0) == 44 and b(d, 8, 16, 896, 1030, 0) == 41 and b(d, 1, 2, 997, 1030, 0) == 41
    assert b(64, 8, 16, 997, 1030, 0) == 41 and b(160, 8, 16, 997, 1030, 0) == 41
    for d in (0, -8, 24, 48, 128, 320):
        assert b(d, 1, 8, 256, 256, 0) < 0
    # the switch is read at every call
    monkeypatch.setenv("BC_ATTN_NO8", "1")
    assert b(40, 2, 8, 8192, 8192, 0) == 44 and b(40, 4, 16, 1000, 1090, 0) == 41 and b(40, 8, 16, 1000, 1090, 0) == 44
    assert b(80, 1, 8, 2048, 2048, 0) == 81                              # (d = 40 only)
    monkeypatch.delenv("BC_ATTN_NO8")
    assert b(40, 2, 8, 8192, 8192, 0) == 84


def test_designed_inputs_make_one_wrong_key_worth_twenty_bars():
    d, heads = 40, 2
    for Nq, Nkv in ((33, 129), (128, 193)):
        power, smax = ac.key_set_power(*ac.make_inputs("leak", 1, heads, d, Nq, Nkv), heads, d, d ** -0.5)
        assert power["extra"] >= ac.POWER and smax <= ac.SCORE_LIMIT, (power, smax)
        power, smax = ac.key_set_power(*ac.make_inputs("drop", 1, heads, d, Nq, Nkv), heads, d, d ** -0.5)
        assert min(power[n] for n in ("last", "first", "tile")) >= ac.POWER and smax <= ac.SCORE_LIMIT, (power, smax)
        # ... which Gaussian inputs do not: a leaked zero key is invisible at any size
        power, _ = ac.key_set_power(*ac.make_inputs("plain", 1, heads, d, Nq, Nkv), heads, d, d ** -0.5)
        assert power["extra"] < 1.0, power
    power, smax = ac.causal_power(*ac.make_ramp_inputs(1, heads, d, 257), heads, d, d ** -0.5)
    assert min(power.values()) >= ac.POWER and smax <= ac.SCORE_LIMIT, (power, smax)
