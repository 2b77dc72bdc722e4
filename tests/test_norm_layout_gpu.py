"""The norm, softmax and layout launches on their own (csrc/norm.hip, the encoder-side half of csrc/elementwise.hip, the row ops of
csrc/sam_ops.hip) against the float64 reference of their operation, in NaN-fenced buffers (tests/norm_layout_common.py: problems, bars,
fences; what that harness sees is shown on the CPU in tests/test_norm_layout_cpu.py).  Every launch goes through the Recorder as the
models record it - Recorder.layernorm / groupnorm / dup_halves, Recorder.call for the rest - one launch (GroupNorm: its launches) per
segment, replayed once.  Every problem prints a MARGIN line: max error over its derived bar, fence elements found untouched."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from blobctrl_amd import _lib  # noqa: E402
from tests import norm_layout_common as nl  # noqa: E402

DEV = torch.device("cuda:0")


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def record(rec, prob):
    """The launch of `prob` as the models record it."""
    a, v, op = prob.args, prob.views, prob.op
    out = prob.outs[0][1].t
    keep = tuple(x.parent for x in v.values()) + tuple(o.parent for _, o, _, _ in prob.outs)
    if op == "layernorm":
        rec.layernorm(v["x"].t, a["rows"], a["C"], v["gamma"].t, v["beta"].t, a["eps"], out=out, ldx=a["ldx"], ldy=a["ldy"])
    elif op == "softmax":
        rec.call("bc_softmax_rows", v["x"].t, a["rows"], a["cols"], a["ld"], kind="softmax", keep=keep)
    elif op == "groupnorm":
        x1, x2 = v["x1"].t, v["x2"].t if a["C2"] else None
        if a["stats"] == "encoded":                            # a test standing in for the producers: one slot per channel
            for x, name in ((x1, "tot1"), (x2, "tot2")):
                if x is not None:
                    rec.tots[x.data_ptr()] = v[name].t
                    rec.tots_per_channel.add(id(v[name].t))
        rec.groupnorm(x1, a["C1"], x2, a["C2"], a["B"], a["HW"], a["G"], a["eps"], v["gamma"].t, v["beta"].t, a["silu"], out=out)
    elif op == "gn_stats":
        rec.call("bc_gn_stats", v["x"].t, a["C"], a["B"], a["HW"], out, kind="gn_stats", keep=keep)
    elif op == "to_nhwc":
        rec.call("bc_nchw_to_nhwc_f16", v["x"].t, 1 if a["f32"] else 0, a["B"], a["C"], a["HW"], a["Cpad"], out, keep=keep)
    elif op == "to_nchw":
        rec.call("bc_nhwc_to_nchw", v["x"].t, a["B"], a["C"], a["HW"], a["ld"], out, 1 if a["f32"] else 0, keep=keep)
    elif op == "patchify":
        rec.call("bc_patchify", v["px"].t, a["B"], a["H"], a["W"], a["patch"], a["Kpad"], out, keep=keep)
    elif op == "add_cls_pos":
        rec.call("bc_add_cls_pos", v["patches"].t, v["cls"].t, v["pos"].t, a["B"], a["T"], a["D"], out, keep=keep)
    elif op == "embed_tokens":
        rec.call("bc_embed_tokens", a["ids"], v["tok"].t, v["pos"].t, a["B"], a["T"], a["D"], a["vocab"], out, keep=keep + (a["ids"],))
    elif op == "gaussian_sample":
        rec.call("bc_gaussian_sample", v["mom"].t, v["noise"].t, a["B"], a["Cz"], a["HW"], nl.SCALE, out, keep=keep)
    elif op == "silu":
        rec.call("bc_silu", v["x"].t, out, a["n"], keep=keep)
    elif op == "add_pos":
        rec.call("bc_add_pos", v["x"].t, v["pos"].t, a["B"], a["T"], a["D"], out, keep=keep)
    elif op == "add_rows":
        rec.call("bc_add_rows", v["a"].t, v["b"].t, a["rows"], a["b_rows"], a["C"], out, keep=keep)
    elif op == "act_rows":
        rec.call("bc_act_rows", v["x"].t, a["n"], a["act"], keep=keep)
    elif op == "dup_halves":
        rec.dup_halves([(o.t, nbytes) for (_, o, _, _), nbytes in zip(prob.outs, a["bytes"])])
    else:
        assert op == "memset_zero", op
        rec.call("bc_memset_zero", out, a["bytes"], kind="memset", keep=keep)


def launch(prob):
    """One problem in a recorder of its own (Recorder.tots is keyed by address: nothing of an earlier problem may answer for this one).
    Returns the kinds the segment recorded."""
    from blobctrl_amd.launch import Recorder
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    prob.assert_inside()
    prob.prepare()
    rec = Recorder(DEV)
    try:
        seg = rec.begin("launch")
        record(rec, prob)
        seg.run(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return dict(seg.kinds)
    finally:
        rec.close()


def passes(prob):
    kinds = launch(prob)
    worst, checked = prob.verify()
    assert checked > 0, prob.name
    print(f"MARGIN {prob.op} | {prob.name}: max err/bar {worst:.3f} | {checked} sentinel elements checked")
    return kinds


def refuses(prob, message):
    """The launch returns non-zero with the library's message and leaves every output bit as it was."""
    with pytest.raises(_lib.BlobCtrlHipError, match=message):
        launch(prob)
    torch.cuda.synchronize()
    assert prob.untouched(), f"{prob.name}: a refused launch wrote"


# ---------------------------------------------------------------------------------------------------- LayerNorm, softmax
@pytest.mark.parametrize("C", nl.LN_WIDTHS)
def test_layernorm(C):
    cases = [c for c in nl.layernorm_cases() if c["C"] == C]
    assert {c["family"] for c in cases} == set(nl.LN_FAMILIES)
    for c in cases:
        passes(nl.layernorm_problem(DEV, **c))


def test_layernorm_refuses_a_row_wider_than_its_registers():
    refuses(nl.layernorm_problem(DEV, C=2056, rows=5, layout="packed", family="unit"), r"bc_layernorm: C=2056 unsupported")


@pytest.mark.parametrize("cols", nl.SM_COLS)
def test_softmax_rows(cols):
    for c in nl.softmax_cases(cols):
        prob = nl.softmax_problem(DEV, **c)
        masked = torch.isinf(prob.views["x"].valid().cpu())
        passes(prob)
        if c["family"] == "masked":                            # exp(-inf) is exactly 0
            assert int(masked.sum()) >= cols // 7 and float(prob.out("p").check(prob.name)[0][masked].abs().max()) == 0.0, prob.name


def test_softmax_rows_refuses_too_many_columns_and_a_short_row_stride():
    refuses(nl.softmax_problem(DEV, 9224, 9, 8, "3g"), r"bc_softmax_rows: cols=9224")
    refuses(nl.softmax_problem(DEV, 520, 9, 0, "3g", ld=512), r"bc_softmax_rows: cols=520")


# ---------------------------------------------------------------------------------------------------- GroupNorm
@pytest.mark.parametrize("route", ["fused", "unfused"])
@pytest.mark.parametrize("shape", nl.GN_SHAPES, ids=[f"{s[0]}+{s[1]}-G{s[2]}-HW{s[3]}" for s in nl.GN_SHAPES])
def test_groupnorm(shape, route, monkeypatch):
    """Both routes: bc_gn_apply_fused, and bc_gn_finalize + bc_gn_apply (BC_GN_UNFUSED, read when the launch is recorded; above 96 channels
    per group the recorder takes it on its own)."""
    if route == "unfused":
        monkeypatch.setenv("BC_GN_UNFUSED", "1")
    else:
        monkeypatch.delenv("BC_GN_UNFUSED", raising=False)
    C1, C2, G, HW = shape
    two_launches = route == "unfused" or (C1 + C2) // G > 96
    for c in nl.groupnorm_cases(shape):
        kinds = passes(nl.groupnorm_problem(DEV, **c))
        apply_kind = "groupnorm" if c["stats"] == "recorded" else "groupnorm_fused_stats"
        assert kinds.get(apply_kind) == 1 and kinds.get("gn_finalize", 0) == (1 if two_launches else 0), (c, kinds)
        assert kinds.get("gn_stats", 0) == ((2 if C2 else 1) if c["stats"] == "recorded" else 0), (c, kinds)


def test_the_fused_groupnorm_refuses_104_channels_per_group():
    prob = nl.groupnorm_problem(DEV, (208, 0, 2, 70), True, "encoded")
    a, v = prob.args, prob.views
    rc_ = _lib.load().bc_gn_apply_fused(v["tot1"].t.data_ptr(), a["C1"], None, 0, v["x1"].t.data_ptr(), None, a["B"], a["HW"], a["G"], a["eps"],
                                        v["gamma"].t.data_ptr(), v["beta"].t.data_ptr(), 1, prob.out("y").t.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc_ != 0 and b"104 channels per group" in _lib.load().bc_last_error() and prob.untouched()


@pytest.mark.parametrize("shape", nl.GS_SHAPES)
def test_gn_stats_adds_to_the_totals_it_finds(shape):
    passes(nl.gn_stats_problem(DEV, shape))


# ---------------------------------------------------------------------------------------------------- layout, embeddings, sample, activations
@pytest.mark.parametrize("entry", ["bc_nchw_to_nhwc_f16", "bc_nhwc_to_nchw", "bc_patchify", "bc_add_cls_pos", "bc_embed_tokens", "bc_gaussian_sample",
                                   "bc_silu", "bc_add_pos", "bc_add_rows", "bc_act_rows", "bc_memset_zero"])
def test_launch(entry):
    """Among the problems of every grid-stride launch is one past its cap of 2048 workgroups; every element is checked."""
    for prob in nl.MAKERS[entry](DEV):
        passes(prob)


def test_nchw_to_nhwc_zeroes_the_pad_lanes():
    prob = nl.to_nhwc_problem(DEV, (2, 5, 33, 16), True)
    passes(prob)
    assert float(prob.out("nhwc").check(prob.name)[0][:, 5:].abs().max()) == 0.0


def test_memset_zero_refuses_a_size_that_is_no_multiple_of_16():
    prob = nl.memset_zero_problem(DEV, 4080)
    prob.args["bytes"] = 4088
    refuses(prob, r"bc_memset_zero: needs a 16-byte aligned pointer and size")


# ---------------------------------------------------------------------------------------------------- dup_halves
def test_dup_halves_through_the_recorder():
    passes(nl.dup_halves_problem(DEV))


def _dup_raw(prob, null_all=False):
    slots = [(None, nl.DUP_NULL_BYTES)] * 6
    if not null_all:
        for (_, o, _, _), nbytes, k in zip(prob.outs, prob.args["bytes"], nl.DUP_SLOTS):
            slots[k] = (o.t.data_ptr(), nbytes)
    rc_ = _lib.load().bc_dup_halves(*[x for s in slots for x in s], stream())
    torch.cuda.synchronize()
    return rc_


def test_dup_halves_compacts_the_null_slots():
    """p1 and p4 null (with a size, as a caller may leave one): slot k of the launch takes pointer AND size of the k-th buffer that is there."""
    prob = nl.dup_halves_problem(DEV)
    prob.assert_inside()
    assert _dup_raw(prob) == 0
    worst, checked = prob.verify()
    print(f"MARGIN dup_halves | raw entry point, p1 and p4 null: max err/bar {worst:.3f} | {checked} sentinel elements checked")
    assert checked == 4 * 2 * 4096


def test_dup_halves_refuses_six_null_slots():
    prob = nl.dup_halves_problem(DEV)
    before = [o.bits.clone() for _, o, _, _ in prob.outs]
    assert _dup_raw(prob, null_all=True) != 0 and b"nothing to copy" in _lib.load().bc_last_error()
    assert all(torch.equal(b, o.bits) for b, (_, o, _, _) in zip(before, prob.outs))
