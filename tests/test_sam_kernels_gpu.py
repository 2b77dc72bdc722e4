"""The kernels of the Segment-Anything path (include/blobctrl_sam.h) one by one, through the C ABI.

bc_attention_relpos is held to the project's attention bar (tests/attention_common.py: 3e-3 + 2e-3 |ref| per element) against float64
softmax(scale Q K^T + rel_h + rel_w) V computed from the fp16-rounded operands, in the layout the model uses: Q and K at column offsets of one
projection buffer, V^T zero padded to the 64-key tile.  Grids 7 x 7 and 14 x 14 end in a ragged key tile, 8 x 12 tells h from w, batch 3
tells a stride error.  Window partition / unpartition are exact copies and are compared bit for bit; the bilinear resize is compared with
F.interpolate on the CPU at 1e-5 of the input's scale."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from blobctrl_amd import _lib  # noqa: E402
from tests import attention_common as ac  # noqa: E402
from tests.common import g  # noqa: E402

NAN16 = 0x7E5A                          # an fp16 NaN bit pattern
GRIDS = [(7, 7), (14, 14), (16, 16), (8, 12), (3, 64)]        # (a 64-wide grid runs the kernel's key-row-per-tile form)
HEADS, BATCH = 2, 3


def _stream():
    return torch.cuda.current_stream().cuda_stream


def nan_buffer(n):
    return torch.full((n,), NAN16, dtype=torch.int16, device="cuda").view(torch.float16)


def bias_reference(q, rh, rw, heads, d, Kh, Kw):
    """float64 rel_h[q][kh] + rel_w[q][kw] of one image from the unscaled query: [heads][N][N]."""
    N = Kh * Kw
    qh = q.double().view(N, heads, d).transpose(0, 1).reshape(heads, Kh, Kw, d)
    ih = torch.arange(Kh)[:, None] - torch.arange(Kh)[None, :] + Kh - 1
    iw = torch.arange(Kw)[:, None] - torch.arange(Kw)[None, :] + Kw - 1
    rel_h = torch.einsum("nhwc,hkc->nhwk", qh, rh.double()[ih])
    rel_w = torch.einsum("nhwc,wkc->nhwk", qh, rw.double()[iw])
    return (rel_h[..., :, None] + rel_w[..., None, :]).reshape(heads, N, N)


def reference(q, k, v, rh, rw, heads, d, Kh, Kw):
    out = []
    for b in range(q.shape[0]):
        s = ac.scores(q[b], k[b], heads, d, d ** -0.5) + bias_reference(q[b], rh, rw, heads, d, Kh, Kw)
        out.append(ac._attend(s, ac._heads_view(v[b], heads, d)))
    return torch.stack(out)


def launch_relpos(q, k, v, rh, rw, heads, d, Kh, Kw, guard=False):
    """q / k / v fp16 [B][N][C] on the CPU -> the kernel's output [B][N][C] (CPU).  Operands are laid out as the model lays them out: one
    [B][N][2 C (+ 8)] projection buffer holding Q | K, V^T [B][C][ldvt] zero padded.  guard: every buffer is carved from NaN-filled memory
    with NaN columns, NaN rows between images and NaN behind the last view; the output buffer must keep its NaN pattern outside the view."""
    lib = _lib.load()
    B, N, Cc = q.shape
    ld = 2 * Cc + (8 if guard else 0)
    rows = N + (3 if guard else 0)                      # rows per image of the projection buffer (the extra ones stay NaN)
    ldvt = (N + 63) // 64 * 64
    qk = nan_buffer(B * rows * ld + 4096).clone()
    qkv = qk[: B * rows * ld].view(B, rows, ld)
    qkv[:, :N, :Cc] = q.cuda()
    qkv[:, :N, Cc:2 * Cc] = k.cuda()
    vbuf = nan_buffer(B * Cc * ldvt + 4096).clone()
    vt = vbuf[: B * Cc * ldvt].view(B, Cc, ldvt)
    vt.zero_()
    vt[:, :, :N] = v.cuda().transpose(1, 2)
    tabs = nan_buffer((2 * Kh - 1 + 2 * Kw - 1) * d + 4096).clone()
    th, tw = tabs[: (2 * Kh - 1) * d], tabs[(2 * Kh - 1) * d: (2 * Kh - 1 + 2 * Kw - 1) * d]
    th.copy_(rh.reshape(-1).cuda())
    tw.copy_(rw.reshape(-1).cuda())
    ldo, orows = Cc + (8 if guard else 0), N + (2 if guard else 0)
    obuf = nan_buffer(B * orows * ldo + 4096).clone()
    o = obuf[: B * orows * ldo].view(B, orows, ldo)
    rel = torch.full((B * heads * N * (Kh + Kw),), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(lib.bc_attention_relpos(qkv.data_ptr(), qkv.data_ptr() + 2 * Cc, vt.data_ptr(), o.data_ptr(), B, heads, d, Kh, Kw, Kh, Kw, ld, ld,
                                       ldvt, ldo, rows * ld, rows * ld, Cc * ldvt, orows * ldo, d ** -0.5, th.data_ptr(), tw.data_ptr(),
                                       rel.data_ptr(), _stream()), "bc_attention_relpos")
    torch.cuda.synchronize()
    out = o[:, :N, :Cc].cpu()
    if guard:
        keep = obuf.view(torch.int16).clone()
        keep[: B * orows * ldo].view(B, orows, ldo)[:, :N, :Cc] = NAN16
        assert bool((keep == NAN16).all()), "the kernel wrote outside its output view"
    return out


@functools.lru_cache(maxsize=None)
def plain_case(Kh, Kw, d):
    """Gaussian operands and tables (bias std about 1), and their float64 reference: built once per shape."""
    N, Cc = Kh * Kw, HEADS * d
    q, k, v = (g(11 + i, BATCH, N, Cc).half() for i in range(3))
    rh, rw = (g(21, 2 * Kh - 1, d) / math.sqrt(d)).half(), (g(22, 2 * Kw - 1, d) / math.sqrt(d)).half()
    return q, k, v, rh, rw, reference(q, k, v, rh, rw, HEADS, d, Kh, Kw)


@pytest.mark.parametrize("d", [80, 64, 40])
@pytest.mark.parametrize("grid", GRIDS, ids=[f"{a}x{b}" for a, b in GRIDS])
def test_relpos_attention_holds_the_bar(grid, d):
    Kh, Kw = grid
    q, k, v, rh, rw, ref = plain_case(Kh, Kw, d)
    out = launch_relpos(q, k, v, rh, rw, HEADS, d, Kh, Kw)
    ac.assert_within_bar(out, ref, d, f"relpos {Kh}x{Kw} d={d}")


@pytest.mark.parametrize("grid", [(7, 7), (8, 12), (3, 64)], ids=["7x7", "8x12", "3x64"])
def test_relpos_attention_in_nan_filled_memory(grid):
    """NaN columns beside Q | K, NaN rows between the images and behind every view (the V^T padding columns are zero: the kernel's contract).
    The K rows of the ragged last tile (7 x 7: rows 49 .. 63) are then NaN or the next image's: neither may reach the output."""
    Kh, Kw = grid
    q, k, v, rh, rw, ref = plain_case(Kh, Kw, 80)
    out = launch_relpos(q, k, v, rh, rw, HEADS, 80, Kh, Kw, guard=True)
    ac.assert_within_bar(out, ref, 80, f"relpos {Kh}x{Kw} in NaN-filled memory")


@pytest.mark.parametrize("d", [80, 40])
def test_zero_tables_agree_with_plain_attention(d):
    """Rh = Rw = 0 is plain attention.  NOT bit for bit: bc_attention folds the scale into an fp16 query and keeps a lazily moved fp16
    softmax reference, this kernel scales the fp32 product and subtracts the running maximum - two roundings of the same sum.  Both lie within
    the bar of the float64 reference, and they must lie within one bar of each other."""
    Kh, Kw = 14, 14
    N, Cc = Kh * Kw, HEADS * d
    q, k, v, _, _, _ = plain_case(Kh, Kw, d)
    zh, zw = torch.zeros(2 * Kh - 1, d).half(), torch.zeros(2 * Kw - 1, d).half()
    ours = launch_relpos(q, k, v, zh, zw, HEADS, d, Kh, Kw)
    ref = ac.reference(q, k, v, HEADS, d, d ** -0.5)
    ac.assert_within_bar(ours, ref, d, f"zero tables d={d}")
    lib = _lib.load()
    ldvt = (N + 63) // 64 * 64
    qc, kc = q.cuda(), k.cuda()
    vt = torch.zeros(BATCH, Cc, ldvt, dtype=torch.float16, device="cuda")
    vt[:, :, :N] = v.cuda().transpose(1, 2)
    o = torch.zeros(BATCH, N, Cc, dtype=torch.float16, device="cuda")
    _lib.check(lib.bc_attention(qc.data_ptr(), kc.data_ptr(), vt.data_ptr(), o.data_ptr(), BATCH, HEADS, d, N, N, Cc, Cc, ldvt, Cc, N * Cc, N * Cc,
                                Cc * ldvt, N * Cc, d ** -0.5, _stream()), "bc_attention")
    torch.cuda.synchronize()
    w, where = ac.worst(ours, o.cpu().double())
    print(f"zero tables vs bc_attention d={d}: worst difference {w:.3f} bars at {where}")
    assert w <= 1.0


@pytest.mark.parametrize("axis", ["h", "w"])
def test_a_bias_that_selects_the_next_row_or_column_of_keys(axis):
    """Rw = 0 and Rh zero except the row that pairs query row qh with key row qh + 1, where it is aligned with a component every query carries:
    the bias is about +16 there and 0 elsewhere, so a query follows V of the key row below it.  V holds the key's row number, so the output is
    qh + 1.  (Then the same with the roles of h and w swapped.)  On the non-square 8 x 12 grid an h / w swap cannot pass."""
    Kh, Kw, d = 8, 12, 80
    N, Cc = Kh * Kw, HEADS * d
    u = ac.sign_vector(d, HEADS)
    q = (0.3 * g(31, BATCH, N, Cc) + 0.5 * u).half()
    k = (0.3 * g(32, BATCH, N, Cc)).half()
    kh, kw = torch.arange(N) // Kw, torch.arange(N) % Kw
    coord, size = (kh, Kh) if axis == "h" else (kw, Kw)
    v = coord.float()[None, :, None].expand(BATCH, N, Cc).contiguous().half()
    tab = torch.zeros(2 * size - 1, d)
    tab[size - 2] = u[:d] * (16.0 / (0.5 * d))             # table row (q - k + size - 1) at k = q + 1
    zero_h, zero_w = torch.zeros(2 * Kh - 1, d).half(), torch.zeros(2 * Kw - 1, d).half()
    rh, rw = (tab.half(), zero_w) if axis == "h" else (zero_h, tab.half())
    ref = reference(q, k, v, rh, rw, HEADS, d, Kh, Kw)
    follows = coord < size - 1                              # (queries of the last row / column have no such key)
    assert float((ref[:, follows] - (coord[follows] + 1).double()[None, :, None]).abs().max()) < 0.05, "the designed bias does not select"
    out = launch_relpos(q, k, v, rh, rw, HEADS, d, Kh, Kw)
    ac.assert_within_bar(out, ref, d, f"selecting bias along {axis}")
    assert float((out[:, follows].double() - (coord[follows] + 1).double()[None, :, None]).abs().max()) < 0.05 + ac.BAR_ATOL + ac.BAR_RTOL * size


# ------------------------------------------------------------------------------------------------------------ windows
def torch_partition(x, H, W, ws):
    B, _, Cc = x.shape
    ph, pw = (ws - H % ws) % ws, (ws - W % ws) % ws
    xp = F.pad(x.view(B, H, W, Cc), (0, 0, 0, pw, 0, ph))
    Hp, Wp = H + ph, W + pw
    return xp.view(B, Hp // ws, ws, Wp // ws, ws, Cc).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, Cc)


@pytest.mark.parametrize("H,W,ws", [(64, 64, 14), (16, 16, 7), (12, 12, 5), (9, 13, 4)])
def test_window_partition_round_trip_is_exact_and_padded_rows_are_zero(H, W, ws):
    lib = _lib.load()
    B, Cc = 2, 40
    # the input's allocation ends at its last real row: nothing behind it may be needed
    x = (g(41, B, H * W, Cc)).half().cuda().clone()
    assert x.untyped_storage().nbytes() == x.numel() * 2
    nW = -(-H // ws) * -(-W // ws)
    win = nan_buffer(B * nW * ws * ws * Cc).view(B * nW, ws * ws, Cc)
    _lib.check(lib.bc_window_partition(x.data_ptr(), B, H, W, Cc, ws, win.data_ptr(), _stream()), "bc_window_partition")
    want = torch_partition(x, H, W, ws)
    torch.cuda.synchronize()
    assert torch.equal(win.view(torch.int16), want.view(torch.int16))
    padded = torch_partition(torch.ones_like(x), H, W, ws) == 0
    assert bool((win[padded].view(torch.int16) == 0).all()) and int(padded.sum()) == (B * nW * ws * ws - B * H * W) * Cc
    res = g(42, B, H * W, Cc).half().cuda()
    out = nan_buffer(B * H * W * Cc).view(B, H * W, Cc)
    _lib.check(lib.bc_window_unpartition(win.data_ptr(), res.data_ptr(), B, H, W, Cc, ws, out.data_ptr(), _stream()), "bc_window_unpartition")
    torch.cuda.synchronize()
    assert torch.equal(out, (x.float() + res.float()).half())
    zero = torch.zeros_like(res)
    _lib.check(lib.bc_window_unpartition(win.data_ptr(), zero.data_ptr(), B, H, W, Cc, ws, out.data_ptr(), _stream()), "bc_window_unpartition")
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), x.view(torch.int16)), "partition -> unpartition is not the identity"


# ------------------------------------------------------------------------------------------------------------ bilinear resize
def _resize(src, crop, size, threshold=None):
    lib = _lib.load()
    N, Cc, H, W = src.shape
    s = src.cuda().contiguous()
    out = torch.empty(N, Cc, size[0], size[1], dtype=torch.uint8 if threshold is not None else torch.float32, device="cuda")
    _lib.check(lib.bc_bilinear_resize_f32(s.data_ptr(), N * Cc, H, W, crop[0], crop[1], size[0], size[1], 0 if threshold is None else 1,
                                          0.0 if threshold is None else threshold, out.data_ptr(), _stream()), "bc_bilinear_resize_f32")
    torch.cuda.synchronize()
    return out.cpu()


def test_bilinear_resize_matches_interpolate():
    a = g(51, 1, 3, 64, 64) * 7.0
    up = _resize(a, (64, 64), (256, 256))
    ref = F.interpolate(a, size=(256, 256), mode="bilinear", align_corners=False)
    scale = float(a.abs().max())
    assert float((up - ref).abs().max()) <= 1e-5 * scale
    b = g(52, 2, 2, 256, 256) * 3.0
    ref = F.interpolate(b[..., :192, :256], size=(150, 200), mode="bilinear", align_corners=False)
    got = _resize(b, (192, 256), (150, 200))
    scale = float(b.abs().max())
    assert float((got - ref).abs().max()) <= 1e-5 * scale
    mask = _resize(b, (192, 256), (150, 200), threshold=0.0)
    sure = ref.abs() > 1e-5 * scale
    assert float((~sure).float().mean()) <= 1e-3
    assert torch.equal(mask[sure].bool(), ref[sure] > 0)
