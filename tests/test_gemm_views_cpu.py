"""The GEMM / convolution view harness (tests/gemm_views_common.py) sees what it claims to see - shown without a device: a torch statement of
the kernel passes, and each mistake a kernel can make (a store or a read outside its views) fails with the message that names it.  Also: the
NaN cases of tests.common.close, and the eligibility of every BC_TILE_GW* / BC_TILE_G256 / halo case of the GPU tables for its tile."""
import pytest
import torch

from tests import gemm_views_common as gv
from tests.common import close, g

CPU = torch.device("cpu")


# ---------------------------------------------------------------------------------------------------- close
def _pair():
    ref = g(1, 64, 48)
    return ref.clone(), ref


def test_close_passes_an_output_inside_the_bar():
    out, ref = _pair()
    close(out + 1e-3, ref, what="inside the bar")
    close(out * (1 + 1e-3), ref, what="inside the relative bar")
    with pytest.raises(AssertionError, match="off, max err"):
        close(out + 1e-2, ref, what="outside the bar")


def test_close_fails_an_all_nan_output():
    out, ref = _pair()
    with pytest.raises(AssertionError, match=f"{ref.numel()}/{ref.numel()} non-finite"):
        close(torch.full_like(out, float("nan")), ref, what="all NaN")


@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf")])
def test_close_fails_one_non_finite_element(value):
    out, ref = _pair()
    out[17, 5] = value
    with pytest.raises(AssertionError, match=f"1/{ref.numel()} non-finite"):
        close(out, ref, what="one element")
    with pytest.raises(AssertionError, match="non-finite"):
        close(out.half(), ref, rtol=0, atol=1e9, what="one element, fp16, a bar nothing finite can miss")


# ---------------------------------------------------------------------------------------------------- the harness against emulated kernels
def dense_prob(flavour="vec"):
    """The generic kernel's ragged case: M, N and K no multiple of a tile, + bias + R."""
    return gv.dense_problem(f"emulated-dense/{flavour}", CPU, flavour, M=130, N=72, K=200, family="generic", R=True)


def conv_prob(flavour="vec"):
    return gv.conv_problem(f"emulated-conv/{flavour}", CPU, flavour, B=2, H=8, W=16, Cin=64, Cout=160, family="halo")


def run(prob, mutation=None):
    prob.assert_inside()
    prob.reset()
    gv.emulate(prob, mutation)
    return prob.verify()


@pytest.mark.parametrize("flavour", gv.FLAVOURS)
@pytest.mark.parametrize("make", [dense_prob, conv_prob])
def test_the_correct_emulation_passes(make, flavour):
    prob = make(flavour)
    worst, checked = run(prob)
    assert worst < 0.5 and checked > 256 * prob.outs[0][1].ld              # (fp16 rounding of the output only; at least one tile of guard rows)
    assert not prob.untouched()


# mutation -> (problem, the message of the failure, the first offending (row, col) where the harness reports one)
M_, N_ = 130, 72
# (store_vec8: 7 elements per row at ld = N + 8; at ld = N + 4 three of them land in the next row's first columns, inside the view)
CAUGHT = [("store_vec8", dense_prob, rf"({M_ * 7}|{M_ * 4 + 3}) elements outside the view were written, first at \(row 0, col {N_}\)"),
          ("rows_round64", dense_prob, rf"{(192 - M_) * N_} elements outside the view were written, first at \(row {M_}, col 0\)"),
          ("skip_one", dense_prob, rf"1 elements of the view were left unwritten, first at \(row {M_ // 2}, col {N_ // 3}\)"),
          ("k_round64", dense_prob, rf"{M_ * N_} non-finite elements in the view \(a leak\), first at \(row 0, col 0\)"),
          ("row_M", dense_prob, rf"{N_} non-finite elements in the view \(a leak\), first at \(row {M_ - 1}, col 0\)"),
          ("bias_lane", dense_prob, rf"{M_} non-finite elements in the view \(a leak\), first at \(row 0, col {N_ - 1}\)"),
          # image 0, output row 0: every pixel's three upper taps come from the guard pixels in front of the image
          ("halo_unchecked", conv_prob, rf"{16 * 160} non-finite elements in the view \(a leak\), first at \(row 0, col 0\)")]


@pytest.mark.parametrize("flavour", gv.FLAVOURS)
@pytest.mark.parametrize("mutation,make,message", CAUGHT, ids=[c[0] for c in CAUGHT])
def test_every_mistake_is_caught(mutation, make, message, flavour):
    with pytest.raises(AssertionError, match=message):
        run(make(flavour), mutation)


def test_every_mutation_of_the_emulation_is_exercised():
    assert sorted(c[0] for c in CAUGHT) == sorted(gv.MUTATIONS)


def test_a_store_in_front_of_the_view_is_reported_with_a_negative_row():
    prob = dense_prob()
    run(prob)
    o = prob.outs[0][1]
    o.bits[o.offset - o.ld + 3] = 0
    with pytest.raises(AssertionError, match=r"1 elements outside the view were written, first at \(row -1, col 3\)"):
        prob.verify()


def test_fp32_and_transposed_outputs_use_their_own_sentinel_and_grid():
    p32 = gv.dense_problem("f32", CPU, "scalar", M=33, N=8, K=8, family="generic", out_mode="f32")
    o = p32.outs[0][1]
    assert o.bits.dtype == torch.int32 and o.ld == 12 and o.offset % 2 == 1 and p32.outs[0][3:] == (1e-4, 1e-4)
    pt = gv.dense_problem("t", CPU, "vec", M=231, N=8, K=8, family="generic", out_mode="f16t", rpb=77, ldc=80, extra=5)
    ot, ref = pt.outs[0][1], pt.outs[0][2]
    assert (ot.rows, ot.width, ot.ld) == (3 * 8, 77, 80) and tuple(ref.shape) == (24, 77)
    for o_ in (o, ot):
        assert o_.untouched()
        o_.assert_inside()


# ---------------------------------------------------------------------------------------------------- the GPU case tables
def test_every_gw_g256_and_halo_case_is_eligible_for_its_tile():
    from blobctrl_amd import _lib
    lib = _lib.load()
    n = 0
    for case in gv.gw_cases():
        a = case.args
        assert lib.bc_gemm_wreg_eligible(a["M"], a["N"], a["K"], a.get("C1", 0), a["tile_cfg"]) == 1, case.id
        n += 1
    for case in gv.g256_cases():
        a = case.args
        out_mode = _lib.OUT_F16_T if a.get("out_mode") == "f16t" else _lib.OUT_F16
        assert lib.bc_gemm256_eligible(a["M"], a["N"], a["K"], a.get("C1", 0), out_mode, a.get("rpb", 0) or a["M"], 1 if a.get("want_gn") else 0) == 1, case.id
        n += 1
    for family in ("halo", "wreg"):
        for case in gv.halo_cases(family):
            a = case.args
            up = 2 if a.get("ups") else 1                     # (the entry point takes the size the convolution runs at: BC_TILE_WREG's 2x upsample)
            assert lib.bc_conv_halo_eligible(a["Cin"], a.get("C1", 0), a["Cout"], up * a["H"], up * a["W"], up * a["H"], up * a["W"], 1) == 1, case.id
            n += 1
    assert n == len(gv.gw_cases()) + 6 + 10 + 11


def test_the_case_tables_name_every_family_and_mode_once():
    ids = [c.id for c in gv.generic_cases() + gv.gw_cases() + gv.g256_cases() + gv.halo_cases("halo") + gv.halo_cases("wreg")]
    ids += [gv.fast_case(cfg, mode).id for cfg in range(1, 8) for mode in gv.FAST_MODES]
    assert len(ids) == len(set(ids)) and len(gv.gw_cases()) == 3 * 2 * len(gv.GW_MODES) + 2 * 2
    # the uneven splits the issue names: chunks -> per-split counts of bc_conv_halo_split (cps = ceil(nch / sk))
    for cin, sk, want in ((192, 2, [2, 1]), (320, 2, [3, 2]), (320, 3, [2, 2, 1])):
        nch = cin // 64
        cps = -(-nch // sk)
        assert [min(cps, nch - s * cps) for s in range(-(-nch // cps))] == want


# ---------------------------------------------------------------------------------------------------- refusals at record time
def test_a_refused_problem_is_refused_by_the_recorder_and_every_other_one_records():
    """Recorder.gemm asks the library (bc_gemm_resolve) before it records: a problem bc_gemm refuses raises there with the library's message -
    on a CPU recorder, no launch attempted - and leaves no record, no launch entry and no table behind; every other problem records."""
    from blobctrl_amd import _lib
    from blobctrl_amd.launch import Recorder
    from tests.gemm_records_common import record_view, view_problems
    rec = Recorder(CPU)
    seg = rec.begin("views")
    refused = recorded = 0
    for prob in view_problems():
        n, tables = len(seg.meta), dict(rec._tot_chunk)
        if prob.refused:
            with pytest.raises(_lib.BlobCtrlHipError, match=r"bc_gemm\(gemm\) failed \(rc=1\): bc_gemm"):
                record_view(rec, prob)
            assert len(seg.meta) == n and rec.lib.bc_plan_num_launches(rec.plan, seg.id) == n and rec._tot_chunk == tables, prob.name
            refused += 1
        else:
            record_view(rec, prob)
            assert len(seg.meta) > n and rec.lib.bc_plan_num_launches(rec.plan, seg.id) == len(seg.meta), prob.name
            assert seg.meta[-1]["variant"].startswith(prob.variant), (prob.name, seg.meta[-1]["variant"])
            recorded += 1
    rec.close()
    assert (refused, recorded) == (89, 247)                     # (168 cases in two flavours)
