"""The two named kernels behind bc_attention_ip without a GPU: the header lines and ctypes signatures of bc_attention_ip_path and
bc_attention_ip_with, their place outside every op table, the arguments refused before any launch, and the power of the GPU test's inputs
(tests/test_attention_ip_tiles_gpu.py) to see a wrong key set at its shapes."""
import ctypes as C
import os

import pytest

from blobctrl_amd import _lib
from tests import ip_adapter_common as ip

HERE = os.path.dirname(os.path.abspath(__file__))


def test_header_declares_the_two_entry_points():
    text = open(os.path.join(HERE, "..", "include", "blobctrl_ip.h")).read()
    assert "int bc_attention_ip_path(int d, int T, int rows_per_batch, int heads);" in text
    assert ("int bc_attention_ip_with(int path, const bc_half* Q, const bc_half* K, const bc_half* V, bc_half* O, int B, int rows_per_batch, "
            "int heads, int d,") in text
    assert "int T, int ldq, int ldkv, int ldo, float qk_scale, const float* w, bc_stream stream);" in text
    assert text.index("int bc_attention_ip(") < text.index("int bc_attention_ip_path(") < text.index("int bc_attention_ip_with(")


def test_signatures_are_a_table_of_their_own_and_no_plan_ops():
    assert list(_lib.IP_PATH_SIGNATURES) == ["bc_attention_ip_path", "bc_attention_ip_with"]
    res, args = _lib.IP_PATH_SIGNATURES["bc_attention_ip_with"]
    assert res is C.c_int and args == [C.c_int] + _lib.IP_SIGNATURES["bc_attention_ip"][1]            # the path, then bc_attention_ip's own
    assert _lib.IP_PATH_SIGNATURES["bc_attention_ip_path"] == (C.c_int, [C.c_int] * 4)
    assert (_lib.ATTENTION_IP_SCALAR, _lib.ATTENTION_IP_TILES) == (0, 1)
    for name in _lib.IP_PATH_SIGNATURES:
        assert name not in _lib.EXPORTED_SYMBOLS and name not in _lib.IP_SIGNATURES and not any(name in t for t in _lib._OP_TABLES)
        with pytest.raises(KeyError):
            _lib.op_code(name)
    lib = _lib.load()
    assert lib.bc_attention_ip_with.argtypes == args and lib.bc_attention_ip_path.restype is C.c_int


def _with(lib, path, **over):
    a = dict(Q=0x1000, K=0x2000, V=0x3000, O=0x4000, B=2, rows=72, heads=8, d=40, T=16, ldq=640, ldkv=320, ldo=320, scale=0.158, w=0x5000)
    a.update(over)
    return lib.bc_attention_ip_with(path, a["Q"], a["K"], a["V"], a["O"], a["B"], a["rows"], a["heads"], a["d"], a["T"], a["ldq"], a["ldkv"],
                                    a["ldo"], a["scale"], a["w"], None)


@pytest.mark.parametrize("path,over,word", [
    (1, dict(T=20), b"T=20"), (1, dict(T=4), b"T=4"), (1, dict(T=1), b"T=1"), (1, dict(T=63), b"T=63"),
    (2, {}, b"path=2"), (-1, {}, b"path=-1"),
    (1, dict(T=80), b"T=80"), (1, dict(T=0), b"T=0"), (1, dict(d=24), b"d=24"), (1, dict(Q=None), b"null"), (1, dict(ldo=312), b"ldo=312"),
    (1, dict(V=0x3008), b"16-byte"), (0, dict(T=65), b"T=65"), (0, dict(d=128), b"d=128"),
])
def test_with_refuses_bad_arguments_before_any_launch(path, over, word):
    lib = _lib.load()
    assert _with(lib, path, **over) == 1
    assert b"bc_attention_ip" in lib.bc_last_error() and word in lib.bc_last_error(), lib.bc_last_error()


def test_path_names_a_kernel_for_every_shape_and_the_scalar_one_off_the_tile_grid():
    lib = _lib.load()
    for d in (8, 16, 32, 40, 64, 80, 160):
        for heads in (2, 8):
            for rows in (5, 72, 128, 512, 2048, 8192):
                for T in range(1, _lib.ATTENTION_IP_MAX_T + 1):
                    path = lib.bc_attention_ip_path(d, T, rows, heads)
                    assert path in (0, 1) and (T % 16 == 0 or path == 0), (d, heads, rows, T, path)


def test_path_follows_the_measured_table():
    """profiles/ip_adapter_plus.md: the tiles won with 8 heads of 40, 80 and 160 channels for T = 16, 32, 48, 64 at every row count; the base
    adapter's T = 4 and every unmeasured (heads, d) pair - another split of a measured width included - stay on the scalar kernel."""
    lib = _lib.load()
    for heads, d in ((8, 40), (8, 80), (8, 160)):
        for rows in (128, 512, 2048, 8192):
            assert [lib.bc_attention_ip_path(d, T, rows, heads) for T in (4, 8, 16, 32, 48, 64)] == [0, 0, 1, 1, 1, 1], (heads, d, rows)
    for heads, d in ((4, 80), (2, 160), (16, 40), (2, 8), (2, 40), (8, 8), (8, 64), (2, 64), (8, 32), (8, 16)):
        assert [lib.bc_attention_ip_path(d, T, 512, heads) for T in (4, 16, 64)] == [0, 0, 0], (heads, d)


def test_recorder_names_the_kernel_the_library_picks():
    """The same op and kind on both paths; the listing's variant names the tiles at T = 16, and the T = 4 string is what it was."""
    import torch
    from blobctrl_amd.launch import Recorder
    rec = Recorder(torch.device("cpu"))
    try:
        seg = rec.begin("t")
        q, o, w = torch.zeros(144, 640).half(), torch.zeros(144, 320).half(), torch.ones(1)
        for T in (4, 16, 20, 32):
            kv = torch.zeros(2, T, 320).half()
            rec.attention_ip(q, kv, kv, o, 2, 72, 8, 40, T, 640, 320, 320, 40 ** -0.5, w)
        assert dict(seg.kinds) == {"attention_ip": 4}
        assert [m["variant"] for m in seg.meta] == ["attention_ip_kernel<40>", "attention_ip_tiles_kernel<40,1>", "attention_ip_kernel<40>",
                                                    "attention_ip_tiles_kernel<40,2>"]
    finally:
        rec.close()


@pytest.mark.parametrize("rows", (72, 5))
@pytest.mark.parametrize("heads,d,T", [(2, 8, 16), (8, 40, 48), (2, 160, 64), (8, 80, 32), (2, 64, 32)])
def test_inputs_see_a_wrong_key_set_at_the_tile_shapes(heads, d, T, rows, monkeypatch):
    monkeypatch.setattr(ip, "ROWS", rows)
    q, k, v, o = ip.make_inputs(heads, d, T)
    assert q.shape[1] == rows
    for w in ip.WEIGHTS:
        power = ip.key_set_power(q, k, v, o, heads, d, w)
        assert set(power) == {"dropped", "other_image"} and min(power.values()) >= 0.5, (w, power)
