"""What tests/test_norm_layout_gpu.py rests on, shown without a device (tests/norm_layout_common.py):
1. a torch statement of every launch (`emulate`), storing into the same fenced buffers, passes every problem: the references, the bars and
   the fences agree with a correct launch, and float64 arithmetic rounded once sits at half a bar or less;
2. an fp32 restatement of every launch with a derived bar reaches at most 0.6 of that bar: a correct fp32 kernel has room;
3. every mistake `emulate` can make fails a problem of its launch with the message that names its kind - off the bar, a leak (non-finite),
   left unwritten, written outside the view;
4. the buffers themselves: the input fences are NaN, a changed bit outside an in-place view or in a guard image of a statistics table is
   reported, ulp16 is the fp16 spacing."""
import re

import pytest
import torch

from tests import norm_layout_common as nl

CPU = torch.device("cpu")
OFF, LEAK, UNWRITTEN, STRAY = r"elements off the bar", r"non-finite elements in the view \(a leak\)", r"elements of the view were left unwritten", \
    r"elements outside the view were written"


def run(prob, mutation=None):
    prob.assert_inside()
    nl.emulate(prob, mutation)
    return prob.verify()


# ---------------------------------------------------------------------------------------------------- 1, 2: the clean emulation, the fp32 room
@pytest.mark.parametrize("entry", list(nl.MAKERS))
def test_the_correct_emulation_passes_and_an_fp32_restatement_has_room(entry):
    probs = nl.MAKERS[entry](CPU)
    assert probs
    for prob in probs:
        worst, checked = run(prob)
        assert worst <= 0.51 and checked > 0, (prob.name, worst, checked)
        derived = [label for label, _, _, bar in prob.outs if bar is not None]
        assert sorted(derived) == sorted(prob.f32), prob.name
        for label, o, ref, bar in prob.outs:
            if bar is not None:
                e, _ = nl.over_bar(prob.f32[label], ref, bar, None)
                print(f"{prob.name} [{label}]: fp32 restatement at {e:.3f} of the bar")
                assert e <= 0.6, f"{prob.name} [{label}]: an fp32 restatement at {e:.3f} of the bar"


# ---------------------------------------------------------------------------------------------------- 3. the named mistakes
def _ln(**kw):
    return lambda: nl.layernorm_problem(CPU, **kw)


def _sm(**kw):
    return lambda: nl.softmax_problem(CPU, **kw)


def _gn(shape, **kw):
    return lambda: nl.groupnorm_problem(CPU, shape, kw.pop("silu", True), "encoded", **kw)


BIG_GN, CAT_GN = (1280, 640, 32, 129), (24, 40, 4, 37)
CAUGHT = [
    ("layernorm", "cover_divisor", _ln(C=520, rows=5, layout="packed", family="3g+1"), OFF),
    ("layernorm", "no_eps", _ln(C=512, rows=5, layout="packed", family="eps_visible"), OFF),
    ("layernorm", "one_pass", _ln(C=1024, rows=5, layout="packed", family="mean100"), OFF),
    ("layernorm", "one_pass", _ln(C=1280, rows=37, layout="packed", family="eps_visible"), OFF),
    ("layernorm", "stride_C", _ln(C=520, rows=37, layout="padded", family="3g+1"), LEAK),
    ("layernorm", "stride_C", _ln(C=8, rows=5, layout="pooled", family="unit"), LEAK),
    ("layernorm", "affine_pass0", _ln(C=1032, rows=5, layout="packed", family="3g+1"), OFF),
    ("layernorm", "rows_round4", _ln(C=2048, rows=37, layout="padded", family="unit"), STRAY),
    ("softmax", "no_max", _sm(cols=520, rows=9, pad=8, family="huge"), LEAK),
    ("softmax", "pad_cols", _sm(cols=2056, rows=9, pad=8, family="3g"), LEAK),
    ("softmax", "norm_512", _sm(cols=520, rows=1, pad=0, family="last11"), OFF),
    ("softmax", "last_pass", _sm(cols=4104, rows=9, pad=8, family="3g"), OFF),
    ("softmax", "rows_round4", _sm(cols=9216, rows=9, pad=0, family="masked"), STRAY),
    ("groupnorm", "range_stats", _gn(BIG_GN), OFF),
    ("groupnorm", "range_stats", _gn((2560, 0, 32, 40), silu=False), OFF),
    ("groupnorm", "x1_for_x2", _gn(CAT_GN), LEAK),
    ("groupnorm", "pixel_tail", _gn(CAT_GN), UNWRITTEN),
    ("groupnorm", "pixel_tail", _gn(BIG_GN, silu=False), UNWRITTEN),
    ("groupnorm", "wrong_cpg", _gn(CAT_GN, silu=False), OFF),
    ("gn_stats", "overwrite", lambda: nl.gn_stats_problem(CPU, (2, 8, 1)), OFF),
    ("gn_stats", "slab_tail", lambda: nl.gn_stats_problem(CPU, (2, 520, 129)), OFF),
    ("to_nhwc", "cap", lambda: nl.to_nhwc_problem(CPU, (1, 3, 70000, 8), True), UNWRITTEN),
    ("to_nhwc", "cp_swapped", lambda: nl.to_nhwc_problem(CPU, (2, 3, 35, 8), False), OFF),
    ("to_nhwc", "pad_unwritten", lambda: nl.to_nhwc_problem(CPU, (2, 5, 33, 16), True), UNWRITTEN),
    ("to_nchw", "cap", lambda: nl.to_nchw_problem(CPU, (1, 3, 180000), True), UNWRITTEN),
    ("to_nchw", "cp_swapped", lambda: nl.to_nchw_problem(CPU, (2, 4, 35), False), OFF),
    ("patchify", "cap", lambda: nl.patchify_problem(CPU, (1, 448, 448, 14, 592)), UNWRITTEN),
    ("patchify", "pad_unwritten", lambda: nl.patchify_problem(CPU, (2, 28, 42, 14, 592)), UNWRITTEN),
    ("add_cls_pos", "cap", lambda: nl.add_cls_pos_problem(CPU, (3, 256, 1024)), UNWRITTEN),
    ("add_cls_pos", "pos_by_row", lambda: nl.add_cls_pos_problem(CPU, (2, 5, 16)), LEAK),
    ("embed_tokens", "cap", lambda: nl.embed_tokens_problem(CPU, (3, 700, 2048, 50)), UNWRITTEN),
    ("embed_tokens", "no_clamp", lambda: nl.embed_tokens_problem(CPU, (2, 7, 16, 99)), LEAK),
    ("embed_tokens", "no_clamp", lambda: nl.embed_tokens_problem(CPU, (2, 7, 16, 99), zero_pos=True), LEAK),
    ("embed_tokens", "pos_by_row", lambda: nl.embed_tokens_problem(CPU, (3, 77, 768, 1000)), LEAK),
    ("gaussian_sample", "cap", lambda: nl.gaussian_sample_problem(CPU, (1, 4, 140000)), UNWRITTEN),
    ("gaussian_sample", "no_clamp", lambda: nl.gaussian_sample_problem(CPU, (2, 4, 35)), OFF),
    ("silu", "cap", lambda: nl.silu_problem(CPU, 600000, False), UNWRITTEN),
    ("silu", "cap", lambda: nl.silu_problem(CPU, 600000, True), OFF),
    ("dup_halves", "cap", lambda: nl.dup_halves_problem(CPU), r"slot 5\]: \d+ " + UNWRITTEN),
    ("dup_halves", "uncompacted", lambda: nl.dup_halves_problem(CPU), r"slot 2\]: 8 " + STRAY),
    ("memset_zero", "cap", lambda: nl.memset_zero_problem(CPU, nl.MEMSET_BYTES[-1]), UNWRITTEN),
]


@pytest.mark.parametrize("op,mutation,make,message", CAUGHT, ids=[f"{c[0]}-{c[1]}-{i}" for i, c in enumerate(CAUGHT)])
def test_every_mistake_is_caught_by_kind(op, mutation, make, message):
    prob = make()
    assert prob.op == op
    with pytest.raises(AssertionError, match=message):
        run(prob, mutation)


def test_every_mutation_of_the_emulation_is_exercised():
    assert sorted({(c[0], c[1]) for c in CAUGHT}) == sorted((op, m) for op, ms in nl.MUTATIONS.items() for m in ms)
    assert sorted(nl.MUTATIONS) == sorted(k[len("_emulate_"):] for k in vars(nl) if k.startswith("_emulate_"))


def test_the_designed_inputs_have_the_power_the_bars_need():
    """Dropping eps on the eps-visible rows and a one-pass fp32 variance on the mean-100 rows miss the LayerNorm bar by a wide margin."""
    for m, kw, least in (("no_eps", dict(C=512, rows=5, layout="packed", family="eps_visible"), 1000.0),
                         ("one_pass", dict(C=1024, rows=5, layout="packed", family="mean100"), 3.0)):
        prob = nl.layernorm_problem(CPU, **kw)
        nl.emulate(prob, m)
        _, o, ref, bar = prob.outs[0]
        e, _ = nl.over_bar(o.check(prob.name)[0], ref, bar, torch.float16)
        print(f"{prob.name}: {m} reads {e:.1f} bars")
        assert e > least


# ---------------------------------------------------------------------------------------------------- 4. the buffers
def test_ulp16_is_the_fp16_spacing():
    r = torch.tensor([0.0, 2.0 ** -30, 2.0 ** -24, 2.0 ** -14, 0.75, 1.0, 1.5, 2.0, 1000.0, -65504.0], dtype=torch.float64)
    want = [2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -11, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 0.5, 32.0]
    assert nl.ulp16(r).tolist() == want
    h = torch.tensor([0.75, 1.0, 1000.0], dtype=torch.float16)
    step = (torch.tensor((h.view(torch.int16) + 1).numpy()).view(torch.float16).double() - h.double())
    assert torch.equal(nl.ulp16(h.double()), step)
    # one rounding: 1 + 2^-11 + 2^-30 lies above the midpoint of 1 and 1 + 2^-10; through fp32 it would land on the tie and round to even
    x = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -30], dtype=torch.float64)
    assert float(nl.round_once(x, torch.float16)) == 1.0 + 2.0 ** -10 and float(x.float().half()) == 1.0


def test_the_input_fences_are_nan_everywhere_outside_the_view():
    n = 0
    for prob in [nl.layernorm_problem(CPU, C=520, rows=5, layout="pooled", family="unit"), nl.softmax_problem(CPU, 504, 9, 8, "masked"),
                 nl.groupnorm_problem(CPU, CAT_GN, True, "encoded"), nl.embed_tokens_problem(CPU, (2, 7, 16, 99)),
                 nl.gaussian_sample_problem(CPU, (2, 4, 35)), nl.to_nchw_problem(CPU, (2, 4, 35), True), nl.silu_problem(CPU, 255, False)]:
        for name, v in prob.views.items():
            if isinstance(v, nl.gv.View):
                keep = torch.ones(v.parent.numel(), dtype=torch.bool)
                keep[(v.offset + torch.arange(v.rows)[:, None] * v.ld + torch.arange(v.cols)[None, :]).flatten()] = False
                assert bool(torch.isnan(v.parent[keep]).all()) and int(keep.sum()) >= 2 * v.cols, (prob.name, name)
                n += 1
            else:
                from blobctrl_amd.launch import decode_gn_tot
                d = decode_gn_tot(v.parent)
                assert bool(torch.isnan(d[0]).all()) and bool(torch.isnan(d[-1]).all()) and bool(torch.isfinite(d[1:-1]).all())
    assert n == 14


def test_a_changed_bit_outside_an_in_place_view_is_reported():
    prob = nl.softmax_problem(CPU, 520, 9, 8, "3g")
    run(prob)
    v = prob.views["x"]
    v.parent.view(torch.int16)[v.offset + 520] ^= 1           # the first pad lane of row 0: still NaN, another payload
    with pytest.raises(AssertionError, match=r"1 elements outside the view were written, first at \(row 0, col 520\)"):
        prob.verify()
    prob = nl.silu_problem(CPU, 257, True)
    run(prob)
    prob.views["x"].parent[prob.views["x"].offset - 1] = 0.0
    with pytest.raises(AssertionError, match=r"1 elements outside the view were written, first at \(row -1, col 256\)"):
        prob.verify()


def test_a_changed_guard_image_of_a_statistics_table_is_reported():
    prob = nl.gn_stats_problem(CPU, (2, 8, 1))
    run(prob)
    o = prob.out("totals")
    assert not o.untouched()
    o.parent[3, 7, 5] += 1
    with pytest.raises(AssertionError, match=r"1 elements outside the view were written \(the guard images"):
        prob.verify()


def test_a_store_behind_a_flat_output_is_reported():
    prob = nl.memset_zero_problem(CPU, 4080)
    run(prob)
    o = prob.outs[0][1]
    assert re.match(r"memset_zero 4080", prob.name) and not prob.untouched()
    o.bits[o.offset + 2040] = 0
    with pytest.raises(AssertionError, match=r"1 elements outside the view were written, first at \(row 1, col 0\)"):
        prob.verify()
