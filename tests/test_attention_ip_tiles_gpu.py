"""The two kernels behind bc_attention_ip (csrc/attention_ip.hip) by name, through bc_attention_ip_with: path 0 the scalar kernel, path 1
the MFMA tiles, at the token counts of IP-Adapter Plus (16 per image).  Inputs, float64 reference, NaN fences and the bar are those of
tests/test_ip_adapter_gpu.py (tests/ip_adapter_common.py, tests/attention_common.py); the launches are direct, on the current stream.
B = 2 x 72 rows gives the tiles a ragged last 16-row tile and a tile boundary at the image boundary; 2 x 5 rows is less than one tile."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from blobctrl_amd import _lib  # noqa: E402
from tests import attention_common as ac  # noqa: E402
from tests import ip_adapter_common as ip  # noqa: E402

DEV = torch.device("cuda:0")
TILE_TOKENS = (16, 32, 48, 64)
PATHS = (_lib.ATTENTION_IP_SCALAR, _lib.ATTENTION_IP_TILES)
CASES = [(heads, d, T) for heads in ip.HEADS for d in ip.HEAD_DIMS for T in TILE_TOKENS] + [(2, 64, 32), (2, 16, 16), (8, 32, 48)]   # (every d once)


def raw_args(prob):
    q, k, v, o, B, rows, heads, d, T, ldq, ldkv, ldo, scale, w = prob.args()
    return (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), B, rows, heads, d, T, ldq, ldkv, ldo, scale, w.data_ptr(),
            torch.cuda.current_stream().cuda_stream)


def launch_with(path, prob):
    """One direct launch of the named path (None: bc_attention_ip itself) on the problem's fenced buffers."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    lib = _lib.load()
    prob.assert_inside()
    prob.o.snapshot()
    rc = lib.bc_attention_ip(*raw_args(prob)) if path is None else lib.bc_attention_ip_with(path, *raw_args(prob))
    torch.cuda.synchronize()
    _lib.check(rc, "bc_attention_ip" if path is None else f"bc_attention_ip_with({path})")


def out_bits(prob):
    return prob.o.parent.view(torch.int16).cpu().clone()


@pytest.mark.parametrize("rows", (72, 5))
@pytest.mark.parametrize("heads,d,T", CASES)
def test_both_paths_against_float64(heads, d, T, rows, monkeypatch):
    """Every (heads, d, T) at 2 x 72 and 2 x 5 rows, ldq = 2 C, for w = 1, 0.35 and -0.5, on both paths from the same buffers: within the
    attention bar, no non-finite element in the view, every bit outside the view as it was."""
    monkeypatch.setattr(ip, "ROWS", rows)
    for w in ip.WEIGHTS:
        prob = ip.Problem(DEV, heads, d, T, w)
        q, k, v, o = prob.cpu
        power = ip.key_set_power(q, k, v, o, heads, d, w)
        print(f"attention_ip tiles heads={heads} d={d} T={T} rows={rows} w={w}: rows that see a wrong key set {power}")
        assert power and min(power.values()) >= 0.5, power
        start = prob.o.parent.clone()
        for path in PATHS:
            prob.o.parent.copy_(start)
            launch_with(path, prob)
            what = f"attention_ip path={path} heads={heads} d={d} T={T} rows={rows} w={w}"
            vals, fenced = prob.o.check(what)
            err = ((vals - prob.ref).abs() / ac.bar(prob.ref)).max().item()
            print(f"MARGIN {what}: max err/bar {err:.3f}, {fenced} fence elements untouched")
            assert fenced > 0 and err <= 1.0, f"{what}: max err/bar {err:.3f}"


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("heads,d,T", [(2, 8, 16), (8, 40, 16), (8, 160, 64)])
def test_zero_weight_touches_nothing(heads, d, T, path):
    """w == 0: O and its fences are byte-identical after the launch, on both paths."""
    prob = ip.Problem(DEV, heads, d, T, 0.0)
    launch_with(path, prob)
    assert prob.o.untouched()


def test_tiles_refuse_a_ragged_token_count_before_any_launch():
    """Path 1 with T = 20: an argument error that names T, nothing launched (O byte-identical); path 0 takes the same call."""
    lib = _lib.load()
    prob = ip.Problem(DEV, 8, 40, 20, 1.0)
    prob.o.snapshot()
    assert lib.bc_attention_ip_with(_lib.ATTENTION_IP_TILES, *raw_args(prob)) == 1
    assert b"bc_attention_ip_with" in lib.bc_last_error() and b"T=20" in lib.bc_last_error(), lib.bc_last_error()
    torch.cuda.synchronize()
    assert prob.o.untouched()
    assert lib.bc_attention_ip_path(40, 20, ip.ROWS, 8) == _lib.ATTENTION_IP_SCALAR
    launch_with(_lib.ATTENTION_IP_SCALAR, prob)
    vals, _ = prob.o.check("attention_ip path=0 T=20")
    assert ((vals - prob.ref).abs() / ac.bar(prob.ref)).max().item() <= 1.0


@pytest.mark.parametrize("heads,d,T", [(8, 40, 4), (8, 40, 16), (8, 80, 32), (8, 160, 16), (2, 8, 64), (8, 160, 64), (8, 40, 20)])
def test_the_entry_point_runs_the_path_the_library_names(heads, d, T):
    """bc_attention_ip agrees bit for bit, fences included, with bc_attention_ip_with(bc_attention_ip_path(...)); a T that is no multiple of
    16 is always the scalar kernel's."""
    lib = _lib.load()
    path = lib.bc_attention_ip_path(d, T, ip.ROWS, heads)
    assert path in PATHS and (T % 16 == 0 or path == _lib.ATTENTION_IP_SCALAR)
    prob = ip.Problem(DEV, heads, d, T, 0.35)
    start = prob.o.parent.clone()
    launch_with(None, prob)
    plain = out_bits(prob)
    prob.o.parent.copy_(start)
    launch_with(path, prob)
    assert bool((out_bits(prob) == plain).all()), f"bc_attention_ip differs from path {path} at heads={heads} d={d} T={T}"
    assert not bool((plain == start.view(torch.int16).cpu()).all())                       # (the launch did write)
