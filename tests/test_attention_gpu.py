"""The flash-attention kernel (csrc/attention.hip) against float64 softmax(scale Q K^T) V, on every build `launch_attn` can choose and in the
layout the models use, with inputs that make ONE wrong key worth many bars (tests/attention_common.py).

Every case calls bc_attention / bc_attention_causal directly, asserts which build `bc_attention_build` names for its shape, and holds the
project's attention bar, 3e-3 + 2e-3 |ref| per element.  Where a designed input is used the test first proves, from the float64 reference
alone, that a key set wrong by one key would lie at least 20 bars away."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from blobctrl_amd import _lib  # noqa: E402
from tests import attention_common as ac  # noqa: E402

KINDS = ("plain", "leak", "drop")
SENTINEL = 0x7E5A                       # an fp16 NaN bit pattern: what an output buffer holds where the kernel must not write


def _elems_behind(t):
    st = t.untyped_storage()
    return (st.nbytes() - (t.data_ptr() - st.data_ptr())) // 2


def launch(q, k, vt, o, B, heads, d, Nq, Nkv, ldq, ldk, ldvt, ldo, qbs, kbs, vbs, obs, causal=False):
    """One launch through the C ABI.  Before it runs, the extents the kernel addresses are checked against the tensors' storage."""
    lib = _lib.load()
    Cc = heads * d
    assert _elems_behind(q) >= (B - 1) * qbs + (Nq - 1) * ldq + Cc and _elems_behind(k) >= (B - 1) * kbs + (Nkv - 1) * ldk + Cc
    assert _elems_behind(vt) >= (B - 1) * vbs + Cc * ldvt and _elems_behind(o) >= (B - 1) * obs + (Nq - 1) * ldo + Cc
    fn = lib.bc_attention_causal if causal else lib.bc_attention
    _lib.check(fn(q.data_ptr(), k.data_ptr(), vt.data_ptr(), o.data_ptr(), B, heads, d, Nq, Nkv, ldq, ldk, ldvt, ldo, qbs, kbs, vbs, obs,
                  d ** -0.5, torch.cuda.current_stream().cuda_stream), "bc_attention")
    torch.cuda.synchronize()
    return o


def transposed_v(v, ldvt=None):
    B, Nkv, Cc = v.shape
    ldvt = ldvt or (Nkv + 63) // 64 * 64
    vt = torch.zeros(B, Cc, ldvt, dtype=torch.float16, device=v.device)
    vt[:, :, :Nkv] = v.transpose(1, 2)
    return vt


def dense(q, k, vt, d, B=None, heads=None, Nq=None, causal=False):
    """The kernel on dense [B][N][C] operands; B / heads / Nq below the tensors' own run a sub-problem on the same buffers (same strides)."""
    Bt, Nqt, Cc = q.shape
    Nkv, ldvt = k.shape[1], vt.shape[2]
    B, heads, Nq = B or Bt, heads or Cc // d, Nq or Nqt
    o = torch.full((B, Nq, Cc), SENTINEL, dtype=torch.int16, device="cuda").view(torch.float16)
    launch(q, k, vt, o, B, heads, d, Nq, Nkv, Cc, Cc, ldvt, Cc, Nqt * Cc, Nkv * Cc, Cc * ldvt, Nq * Cc, causal)
    assert bool((o[:, :, heads * d:].view(torch.int16) == SENTINEL).all()), "columns of heads that were not asked for were written"
    return o


def build_of(d, B, heads, Nq, Nkv, causal=0):
    return _lib.load().bc_attention_build(d, B, heads, Nq, Nkv, causal)


def assert_power(kind, q, k, v, heads, d, what):
    """B1: the designed inputs make a key set that is wrong by one key visible - a condition on the inputs, from the reference alone."""
    if kind == "plain":
        return
    power, smax = ac.key_set_power(q, k, v, heads, d, d ** -0.5)
    assert smax <= ac.SCORE_LIMIT, f"{what}: |score| reaches {smax:.1f}"
    for name in (("extra",) if kind == "leak" else ("last", "first", "tile")):
        assert power[name] >= ac.POWER, f"{what}: the '{name}' key set is only {power[name]:.1f} bars from the reference"


@functools.lru_cache(maxsize=None)
def case(kind, B, heads, d, Nq, Nkv):
    """Inputs on the GPU, V^T and the float64 reference of one (kind, shape): built once, shared by the tests that need it, never modified."""
    q, k, v = (t.cuda() for t in ac.make_inputs(kind, B, heads, d, Nq, Nkv))
    assert_power(kind, q, k, v, heads, d, f"{kind} inputs d={d} Nq={Nq} Nkv={Nkv}")
    return q, k, transposed_v(v), ac.reference(q, k, v, heads, d, d ** -0.5)


@pytest.fixture(autouse=True)
def default_builds(monkeypatch):
    monkeypatch.delenv("BC_ATTN_NO8", raising=False)


# ------------------------------------------------------------------------------------------------ B2: every instantiation
# (build, d, B, heads, Nq, Nkv, BC_ATTN_NO8).  B and heads are the smallest the dispatch thresholds allow: 84 needs ceil(Nq / 256) heads B >=
# 256, 44 needs ceil(Nq / 128) heads B >= 1024 (so d = 40 under BC_ATTN_NO8 needs B = 8 at 16 heads and 1000 queries: B = 4 gives 512).
BUILD_CASES = [(84, 40, 4, 16, 1000, 1090, False), (44, 40, 8, 16, 1000, 1090, True),
               (44, 8, 8, 16, 997, 1030, False), (44, 16, 8, 16, 997, 1030, False), (44, 32, 8, 16, 997, 1030, False)]
# d = 80: an even number of full key tiles and no tail, an odd number and no tail, a ragged tail - on the 8-wave and the 4-wave build
BUILD_CASES += [(81, 80, 1, 2, 512, n, False) for n in (1024, 1088, 1090)] + [(41, 80, 1, 2, 511, n, False) for n in (1024, 1088, 1090)]
BUILD_CASES += [(41, 64, 1, 2, 130, 1030, False), (41, 160, 1, 2, 64, 1100, False)]


@pytest.mark.parametrize("build,d,B,heads,Nq,Nkv,no8", BUILD_CASES, ids=[f"build{c[0]}-d{c[1]}-Nq{c[4]}-Nkv{c[5]}" for c in BUILD_CASES])
def test_every_build_holds_the_bar_on_plain_leak_and_drop_inputs(build, d, B, heads, Nq, Nkv, no8, monkeypatch):
    if no8:
        monkeypatch.setenv("BC_ATTN_NO8", "1")
    assert build_of(d, B, heads, Nq, Nkv) == build
    for kind in KINDS:
        q, k, vt, ref = case(kind, B, heads, d, Nq, Nkv)
        ac.assert_within_bar(dense(q, k, vt, d), ref, d, f"build {build} d={d} B={B} heads={heads} Nq={Nq} Nkv={Nkv} {kind}")


# ------------------------------------------------------------------------------------------------ B3: builds agree bit for bit
# Per (batch, head, query) the arithmetic does not depend on the grid or on which queries share a wave (every lane moves its own m_ref), so
# two builds on the same buffers must produce the same bits.
def test_d40_builds_84_44_and_41_agree_bit_for_bit(monkeypatch):
    d, B, heads, Nq, Nkv = 40, 8, 16, 1000, 1090
    for kind in KINDS:
        q, k, vt, _ = case(kind, B, heads, d, Nq, Nkv)
        monkeypatch.delenv("BC_ATTN_NO8", raising=False)
        assert build_of(d, B, heads, Nq, Nkv) == 84 and build_of(d, 1, 2, Nq, Nkv) == 41
        o84, o41 = dense(q, k, vt, d), dense(q, k, vt, d, B=1, heads=2)
        monkeypatch.setenv("BC_ATTN_NO8", "1")
        assert build_of(d, B, heads, Nq, Nkv) == 44
        o44 = dense(q, k, vt, d)
        assert torch.equal(o84, o44), f"{kind}: builds 84 and 44 differ at {int((o84 != o44).sum())} elements"
        assert torch.equal(o84[:1, :, :2 * d], o41[:, :, :2 * d]), f"{kind}: builds 84 and 41 differ"


@pytest.mark.parametrize("d", [8, 16, 32])
def test_small_d_build_44_agrees_with_41_bit_for_bit(d):
    B, heads, Nq, Nkv = 8, 16, 997, 1030
    assert build_of(d, B, heads, Nq, Nkv) == 44 and build_of(d, 1, 2, Nq, Nkv) == 41
    for kind in KINDS:
        q, k, vt, _ = case(kind, B, heads, d, Nq, Nkv)
        o44, o41 = dense(q, k, vt, d), dense(q, k, vt, d, B=1, heads=2)
        assert torch.equal(o44[:1, :, :2 * d], o41[:, :, :2 * d]), f"{kind}: builds 44 and 41 differ"


@pytest.mark.parametrize("Nkv", [1024, 1088, 1090])
def test_d80_build_81_agrees_with_41_bit_for_bit(Nkv):
    d, B, heads = 80, 1, 2
    assert build_of(d, B, heads, 512, Nkv) == 81 and build_of(d, B, heads, 511, Nkv) == 41
    for kind in KINDS:
        q, k, vt, _ = case(kind, B, heads, d, 512, Nkv)
        o81, o41 = dense(q, k, vt, d), dense(q, k, vt, d, Nq=511)
        assert torch.equal(o81[:, :511], o41), f"{kind}: builds 81 and 41 differ at {int((o81[:, :511] != o41).sum())} elements"


# ------------------------------------------------------------------------------------------------ B4: tile edges, default 4-wave build
# Nkv: one tile that is only a tail; one full tile; the two-tile trip with and without a further prefetch; the odd-full-tile branch - each
# with and without a tail.  Nq: a single query, one 32-query block with and without a ragged end, a full workgroup and one query more.
@pytest.mark.parametrize("d", [8, 16, 32, 40, 64, 80, 160])
def test_tile_edges_on_the_default_build(d):
    B, heads = 1, 2
    failures = []
    for Nkv in (1, 63, 64, 65, 127, 128, 129, 192, 193):
        for Nq in (1, 31, 32, 33, 128, 129):
            assert build_of(d, B, heads, Nq, Nkv) == 41
            for kind in (("drop" if Nkv >= 65 else "plain"), "leak"):
                what = f"d={d} Nq={Nq} Nkv={Nkv} {kind}"
                q, k, v = (t.cuda() for t in ac.make_inputs(kind, B, heads, d, Nq, Nkv))
                assert_power(kind, q, k, v, heads, d, what)
                w, (b, qi, c) = ac.worst(dense(q, k, transposed_v(v), d), ac.reference(q, k, v, heads, d, d ** -0.5))
                if w > 1.0:
                    failures.append(f"{what}: worst err/bar {w:.2f} at (b={b}, head={c // d}, query={qi}, column={c % d})")
    assert not failures, f"{len(failures)} shapes off the bar:\n" + "\n".join(failures)


# ------------------------------------------------------------------------------------------------ B5: causal edges
# The tile-skip bound min(Nq, 128 qblk + 128) is crossed at 128 / 129 and 256 / 257.  Ramp inputs: the diagonal key is every query's heaviest,
# so a mask that is off by one key in either direction moves every 32-query block by tens of bars (asserted from the reference alone).
@pytest.mark.parametrize("d", [8, 16, 40, 64])
def test_causal_edges_with_ramp_inputs(d):
    B, heads = 2, 2
    failures = []
    for N in (1, 63, 64, 65, 77, 128, 129, 200, 256, 257):
        what = f"causal d={d} N={N}"
        assert build_of(d, B, heads, N, N, 1) == 41
        q, k, v = (t.cuda() for t in ac.make_ramp_inputs(B, heads, d, N))
        power, smax = ac.causal_power(q, k, v, heads, d, d ** -0.5)
        assert smax <= ac.SCORE_LIMIT, f"{what}: |score| reaches {smax:.1f}"
        assert N == 1 or min(power.values()) >= ac.POWER, f"{what}: a mask off by one key is only {power} bars from the reference"
        w, (b, qi, c) = ac.worst(dense(q, k, transposed_v(v), d, causal=True), ac.reference(q, k, v, heads, d, d ** -0.5, causal=True))
        if w > 1.0:
            failures.append(f"{what}: worst err/bar {w:.2f} at (b={b}, head={c // d}, query={qi}, column={c % d})")
    assert not failures, f"{len(failures)} sizes off the bar:\n" + "\n".join(failures)


# ------------------------------------------------------------------------------------------------ B6: the models' layout, with canaries
POISON = 6e4


@pytest.mark.parametrize("d,B,heads,Nq,Nkv,ldvt,build", [(40, 2, 2, 300, 77, 128, 41),          # cross-attention to the 77 prompt tokens
                                                          (64, 2, 2, 257, 257, None, 41),      # DINOv2's token count
                                                          (80, 1, 2, 1090, 1090, None, 41),    # >= 1024 keys with a ragged tail
                                                          (80, 1, 2, 1280, 1280, None, 81),    # the 8-wave build
                                                          (160, 2, 2, 130, 130, None, 41)])
def test_production_layout_equals_dense_and_writes_nothing_else(d, B, heads, Nq, Nkv, ldvt, build):
    """Q and K as the two halves of one [B][N + 3][2 C] buffer (self-attention: what the fused q | k projection writes; three poison rows per
    image), V^T with a spare zero tile, O with ldo = C + 8 and rows up to the next multiple of 256, prefilled with a sentinel."""
    Cc = heads * d
    assert build_of(d, B, heads, Nq, Nkv) == build
    kind = "drop" if Nkv >= 65 else "plain"
    q, k, v = (t.cuda() for t in ac.make_inputs(kind, B, heads, d, Nq, Nkv))
    assert_power(kind, q, k, v, heads, d, f"layout d={d}")
    ref = ac.reference(q, k, v, heads, d, d ** -0.5)
    o_dense = dense(q, k, transposed_v(v), d)

    qbuf = torch.full((B, Nq + 3, 2 * Cc), POISON, dtype=torch.float16, device="cuda")
    kbuf = qbuf if Nq == Nkv else torch.full((B, Nkv + 3, 2 * Cc), POISON, dtype=torch.float16, device="cuda")
    qbuf[:, :Nq, :Cc] = q
    kbuf[:, :Nkv, Cc:] = k
    ldvt = ldvt or (Nkv + 63) // 64 * 64 + 64
    vt = transposed_v(v, ldvt)
    rows, ldo = (Nq + 255) // 256 * 256, Cc + 8
    obuf = torch.full((B, rows, ldo), SENTINEL, dtype=torch.int16, device="cuda")
    launch(qbuf, kbuf[0, 0, Cc:], vt, obuf.view(torch.float16), B, heads, d, Nq, Nkv, 2 * Cc, 2 * Cc, ldvt, ldo,
           (Nq + 3) * 2 * Cc, (Nkv + 3) * 2 * Cc, Cc * ldvt, rows * ldo)
    out = obuf.view(torch.float16)[:, :Nq, :Cc]
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) <= float(v.abs().max()) + 0.01, "a poison row shows in the output"
    assert torch.equal(out, o_dense), f"{int((out != o_dense).sum())} elements differ from the dense-layout result"
    ac.assert_within_bar(out, ref, d, f"layout d={d} Nq={Nq} Nkv={Nkv}")
    outside = torch.ones_like(obuf, dtype=torch.bool)
    outside[:, :Nq, :Cc] = False
    assert bool((obuf[outside] == SENTINEL).all()), f"{int((obuf[outside] != SENTINEL).sum())} elements outside [0, Nq) x [0, C) were written"
