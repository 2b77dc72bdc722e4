"""The GEMM / convolution view harness (tests/gemm_views_common.py) sees what it claims to see - shown without a device: a torch statement of
the kernel passes, and each mistake a kernel can make (a store or a read outside its views) fails with the message that names it.  Also: the
NaN cases of tests.common.close, the eligibility of every BC_TILE_GW* / BC_TILE_G256 / halo case of the GPU tables for its tile, the kernel
family the library resolves every front-end case to, and what fp16 storage between the launches of the VAE attention leaves of its bar."""
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


GENERIC_CONV = dict(B=2, H=10, W=12, Cin=8, Cout=40, family="generic", lda_pad=0)


def nopad_prob(flavour="vec"):
    """The VAE encoder's downsampler at an even size: output row 4 / column 5 read the bottom / right pad (input row 10, column 12)."""
    return gv.conv_problem(f"emulated-nopad_lo/{flavour}", CPU, flavour, **dict(GENERIC_CONV, stride=2, nopad_lo=True))


def nopad_odd_prob(flavour="vec"):
    return gv.conv_problem(f"emulated-nopad_lo-odd/{flavour}", CPU, flavour, **dict(GENERIC_CONV, H=9, W=11, stride=2, nopad_lo=True))


def stride2_prob(flavour="vec"):
    return gv.conv_problem(f"emulated-stride2/{flavour}", CPU, flavour, **dict(GENERIC_CONV, stride=2))


def size_prob(flavour="vec"):
    """5 x 6 -> 8 x 9: floor(i * 5 / 8) and i >> 1 differ from i = 5 on."""
    return gv.conv_problem(f"emulated-size/{flavour}", CPU, flavour, **dict(GENERIC_CONV, H=5, W=6, size=(8, 9)))


def size_9x11_prob(flavour="vec"):
    return gv.conv_problem(f"emulated-size9x11/{flavour}", CPU, flavour, **dict(GENERIC_CONV, H=5, W=6, size=(9, 11)))


def ups_prob(flavour="vec"):
    return gv.conv_problem(f"emulated-ups/{flavour}", CPU, flavour, **dict(GENERIC_CONV, H=5, W=6, ups=True))


def f32_conv_prob(flavour="vec"):
    return gv.conv_problem(f"emulated-f32/{flavour}", CPU, flavour, **dict(GENERIC_CONV, H=9, W=11, Cout=3, out_mode="f32"))


def residual_conv_prob(flavour="vec"):
    return gv.conv_problem(f"emulated-R/{flavour}", CPU, flavour, **dict(GENERIC_CONV, H=9, W=11, Cin=24, Cout=8, R=True))


def chain_prob(flavour="vec", act="gelu"):
    """(acc + bias) -> act -> colscale -> alpha -> the per-image entry of step 1 of a [2][2] table -> + R."""
    return gv.dense_problem(f"emulated-chain-{act}/{flavour}", CPU, flavour, M=130, N=72, K=200, family="generic", act=act, colscale=True,
                            alpha=0.5, rpb=65, alpha_table=(2, 1, True), R=True)


def quick_gelu_prob(flavour="vec"):
    return chain_prob(flavour, "quick_gelu")


def silu_prob(flavour="vec"):
    return chain_prob(flavour, "silu")


def device_scalar_prob(flavour="vec"):
    return gv.dense_problem(f"emulated-alpha_dev/{flavour}", CPU, flavour, M=130, N=72, K=200, family="generic", alpha_table=(2, 1, False))


def attention_prob(flavour="vec"):
    return gv.vae_attention_problem(CPU, 2, 72, 64)


def run(prob, mutation=None):
    prob.assert_inside()
    prob.reset()
    gv.emulate(prob, mutation)
    return prob.verify()


@pytest.mark.parametrize("flavour", gv.FLAVOURS)
@pytest.mark.parametrize("make", [dense_prob, conv_prob, nopad_prob, nopad_odd_prob, stride2_prob, size_prob, size_9x11_prob, ups_prob, f32_conv_prob,
                                  residual_conv_prob, chain_prob, quick_gelu_prob, silu_prob, device_scalar_prob, attention_prob])
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
          ("halo_unchecked", conv_prob, rf"{16 * 160} non-finite elements in the view \(a leak\), first at \(row 0, col 0\)"),
          # the gather origin one pixel up and left: the bounds test still holds, every value is another pixel's
          ("pad_lo_kept", nopad_prob, r"emulated-nopad_lo/\w+ \[C\]: \d+/2400 off, max err"),
          # input row 10 of image 0 is row 0 of image 1 (finite, wrong); of image 1 it is the guard pixels: its output row 4 (6 pixels, rows
          # 54 .. 59 of the view) is NaN in all 40 channels
          ("pad_hi_unchecked", nopad_prob, rf"{6 * 40} non-finite elements in the view \(a leak\), first at \(row {30 + 4 * 6}, col 0\)"),
          ("ups_shift", size_prob, r"emulated-size/\w+ \[C\]: \d+/\d+ off, max err"),
          ("act_swapped", chain_prob, r"emulated-chain-gelu/\w+ \[C\]: \d+/\d+ off, max err"),
          ("scale_before_act", chain_prob, r"emulated-chain-gelu/\w+ \[C\]: \d+/\d+ off, max err"),
          ("alpha_image0", chain_prob, r"emulated-chain-gelu/\w+ \[C\]: \d+/\d+ off, max err"),
          # step 2 of a two-step table: the NaN lanes behind it
          ("alpha_next_step", chain_prob, rf"{M_ * N_} non-finite elements in the view \(a leak\), first at \(row 0, col 0\)"),
          ("w_image0", attention_prob, r"vae-attention-B2-N72-C64 \[image 1: scores\]: \d+/\d+ off, max err")]


def test_the_mistakes_that_move_values_move_the_rows_they_should():
    """alpha_image0 leaves image 0 alone; pad_hi_unchecked on image 0 reads finite pixels of image 1 into output row 4 and column 5 only; at
    5 x 6 -> 9 x 11 a gather that shifts reads the pixels one that scales reads (floor(i * 5 / 9) == i >> 1 for i < 9, floor(i * 6 / 11) for
    i < 11): the case of the issue cannot see that mistake, the 8 x 9 case can."""
    def stored(prob, mutation):
        prob.reset()
        gv.emulate(prob, mutation)
        o = prob.outs[0][1]
        return o.parent.as_strided((o.rows, o.width), (o.ld, 1), o.offset).double()
    p = chain_prob()
    diff = (stored(p, "alpha_image0") - stored(p, None)).abs().amax(1)
    assert float(diff[:65].max()) == 0.0 and float(diff[65:].min()) > 0.0
    p = nopad_prob()
    diff = (stored(p, "pad_hi_unchecked") - stored(p, None))[:30].abs().amax(1).view(5, 6)
    assert float(diff[:4, :5].max()) == 0.0 and float(diff[4].min()) > 0.0 and float(diff[:, 5].min()) > 0.0
    p = size_9x11_prob()
    assert torch.equal(stored(p, "ups_shift"), stored(p, None))
    assert all(i * 5 // 9 == i >> 1 for i in range(9)) and all(i * 6 // 11 == i >> 1 for i in range(11))


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
            if a.get("nopad_lo"):                             # (the refusal that is pinned: the entry point has no such argument)
                assert a["refused"] is True
                continue
            up = 2 if a.get("ups") else 1                     # (the entry point takes the size the convolution runs at: BC_TILE_WREG's 2x upsample)
            assert lib.bc_conv_halo_eligible(a["Cin"], a.get("C1", 0), a["Cout"], up * a["H"], up * a["W"], up * a["H"], up * a["W"], 1) == 1, case.id
            n += 1
    assert n == len(gv.gw_cases()) + 7 + 10 + 11


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
    for prob in view_problems(front_end=True):
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
    assert (refused, recorded) == (89 + 11, 247 + 129)          # (168 cases in two flavours, and the front ends' 70)


def test_every_front_end_case_resolves_to_the_family_its_table_names():
    """A case meant for the generic gather that lands on the fast path - or the reverse - is a failure of the case: what the library resolves
    each of them to, on a CPU recorder, is the family and the mode the table was written for."""
    from blobctrl_amd.launch import Recorder
    from tests.gemm_records_common import record_view, view_cases
    rec = Recorder(CPU)
    seg = rec.begin("views")
    names = {}
    for case in view_cases(front_end=True):
        if not case.front_end:
            continue
        for flavour in gv.FLAVOURS:
            prob = gv.build(case, flavour, CPU)
            if not prob.refused:
                record_view(rec, prob)
                names[prob.name] = seg.meta[-1]["variant"]
    rec.close()
    assert len(names) == 129
    for name, variant in names.items():
        cid = name.split("/")[0]
        if cid.startswith("generic-"):
            mode = "dense" if "conv" not in cid else ("ups" if "size" in cid or "ups" in cid else ("conv2" if "-s2" in cid else "conv1"))
            # (the cost model splits K = 576 of the Cin = 64 case: the generic gather in front of the split-K reducer)
            assert variant.startswith("gemm_kernel<") and variant.replace("+splitk_reduce", "").endswith(f",{mode}>"), (name, variant)
            assert ("+splitk_reduce" in variant) == ("Cin64" in cid), (name, variant)
        elif cid.startswith("fast"):
            cfg, mode = int(cid[4]), cid[6:]
            from blobctrl_amd import _lib
            want = f"gemm_fast_kernel<{_lib.TILE_NAMES[cfg]}," + ("conv2>" if mode.startswith("conv2") else "dense>")
            assert variant == want + ("+splitk_reduce" if mode.endswith("sk3") else ""), (name, variant)
        elif cid.startswith("g256"):
            assert variant.startswith("gemm256_kernel<"), (name, variant)
        else:
            assert variant.startswith("gemm_wreg_kernel<"), (name, variant)


@pytest.mark.parametrize("B,N,C", gv.ATTN_SHAPES)
def test_the_vae_attention_recording_names_the_launches_the_problem_expects(B, N, C):
    """AutoencoderKL._attend - the recording the model uses - on the fenced buffers, on a CPU recorder: three launches per image, Q K^T on
    gemm_fast, P V on the generic kernel where K = pad8(N) is no multiple of 64."""
    from blobctrl_amd.launch import Recorder
    from blobctrl_amd.vae import AutoencoderKL
    prob = gv.vae_attention_problem(CPU, B, N, C)
    prob.assert_inside()
    rec = Recorder(CPU)
    seg = rec.begin("vae_attention")
    AutoencoderKL._attend(rec, prob.views["qk"].t, prob.views["vt"].t, prob.s.t, prob.o.t, B, N, C)
    assert len(seg.meta) == 3 * B
    for i, m in enumerate(seg.meta):
        kind, variant = prob.launches[i % 3]
        assert m["kind"] == kind and m["variant"].startswith(variant) and (variant or not m["variant"]), (i, m)
    assert [seg.meta[i]["variant"].split("<")[0] for i in (0, 2)] == (["gemm_fast_kernel", "gemm_kernel"] if N == 72 else ["gemm_fast_kernel"] * 2)
    rec.close()


# ---------------------------------------------------------------------------------------------------- the floor of the attention chain
@pytest.mark.parametrize("B,N,C", gv.ATTN_SHAPES)
def test_fp16_storage_of_scores_and_probabilities_leaves_half_of_the_attention_bar(B, N, C):
    """The attention bar (3e-3 + 2e-3 |ref|) was set for one fused kernel; the VAE's chain stores fp16 scores and fp16 probabilities in
    between.  What that storage alone costs: float64 arithmetic rounded to fp16 exactly where the three launches store, against the float64
    references.  Measured here (profiles/gemm_views_margins.txt holds the figures): at most half of each stage's bar, so that a kernel has
    the other half for its fp32 accumulation."""
    prob = gv.vae_attention_problem(CPU, B, N, C)
    run(prob)
    print(f"FLOOR {prob.name}: " + ", ".join(f"{st} {prob.worst[st]:.3f}" for st in gv.ATTN_STAGES))
    assert float(prob.refs["scores"].abs().max()) < 8.0          # (the scores of unit-normal q, k: fp16 spacing 2^-8 below 8)
    for st in gv.ATTN_STAGES:
        assert prob.worst[st] <= 0.5, (st, prob.worst[st])


def test_a_write_into_an_inputs_guards_is_seen():
    prob = gv.vae_attention_problem(CPU, 1, 64, 128)
    run(prob)
    v = prob.views["vt"]
    v.parent[v.offset - 1] = 0.0
    with pytest.raises(AssertionError, match="the NaN guards around vt were written"):
        prob.verify()
