"""The cases whose output bits tests/test_attention_ip_bits_gpu.py pins (tests/golden/attention_ip_bits.json), and the digests of their
CPU-made inputs (tests/test_attention_ip_bits_cpu.py).  Nothing here needs a device.

Every case is one launch by name - bc_attention_ip_with / bc_attention_ip_masked_with - at w = 0.35 on the fenced problems of
tests/ip_adapter_common.py and tests/ip_masks_common.py:
  plain, both paths     every CASES entry of tests/test_attention_ip_tiles_gpu.py at 72 and at 5 rows
  plain, scalar only    T = 1, 4, 5, 20 at every (heads, d) of HEADS x HEAD_DIMS
  masked, scalar        every (heads, d) of HEADS_D and HEADS_D_MORE x IMAGES_TP
  masked, tiles         the same wherever Tp % 16 == 0"""
import contextlib
import hashlib
import json
import os

from tests import ip_adapter_common as ip
from tests import ip_masks_common as mc
from tests.test_attention_ip_tiles_gpu import CASES as TILE_CASES

W = 0.35
SCALAR_TOKENS = (1, 4, 5, 20)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_ip_bits.json")


@contextlib.contextmanager
def rows_as(rows):
    """tests/ip_adapter_common.py makes its inputs at its module's ROWS: another row count for the length of a `with`."""
    before, ip.ROWS = ip.ROWS, rows
    try:
        yield
    finally:
        ip.ROWS = before


def cases():
    """[(id, kind, path, parameters)]: kind "plain" with (heads, d, T, rows), kind "masked" with (heads, d, images, Tp)."""
    out = []
    for heads, d, T in TILE_CASES:
        for rows in (72, 5):
            for path in (0, 1):
                out.append((f"plain path={path} heads={heads} d={d} T={T} rows={rows}", "plain", path, (heads, d, T, rows)))
    for heads in ip.HEADS:
        for d in ip.HEAD_DIMS:
            for T in SCALAR_TOKENS:
                out.append((f"plain path=0 heads={heads} d={d} T={T} rows=72", "plain", 0, (heads, d, T, 72)))
    for heads, d in mc.HEADS_D + mc.HEADS_D_MORE:
        for images, Tp in mc.IMAGES_TP:
            for path in ((0, 1) if Tp % 16 == 0 else (0,)):
                out.append((f"masked path={path} heads={heads} d={d} images={images} Tp={Tp}", "masked", path, (heads, d, images, Tp)))
    assert len({c[0] for c in out}) == len(out)
    return out


def digest(*tensors):
    """sha256 over the tensors' bytes, in order."""
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().numpy().tobytes())
    return h.hexdigest()


def rows_of(kind, params):
    """The row count a case's problem is made AND launched at: `with rows_as(rows_of(kind, params))` goes around both."""
    return params[3] if kind == "plain" else mc.ROWS


def cpu_inputs(kind, params):
    """The fp16 tensors a case's Problem is built from (q, k, v, o_in and, masked, the mask), as Problem.cpu holds them."""
    with rows_as(rows_of(kind, params)):
        return ip.make_inputs(*params[:3]) if kind == "plain" else mc.make_inputs(*params)[:5]


def problem(device, kind, params):
    """The case's fenced problem (inside rows_as)."""
    return ip.Problem(device, *params[:3], W) if kind == "plain" else mc.Problem(device, *params, W)


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
