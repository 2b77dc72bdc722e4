"""What tests/test_rowchain_stages_gpu.py rests on, shown without a device (tests/rowchain_stages_common.py):
1. the float64 stage references, chained with a float64 attention and with weights and inputs left unrounded, reproduce the reference's
   Transformer2DModel (tests/golden/blocks.npz, fp32 diffusers) to 1e-5 of the tensor's scale;
2. at the designed inputs each named mistake moves the reference ALONE by more than 5 bars: in every row it concerns; the key-set and
   scale mistakes by more than 5 bars somewhere and out of the bar (more than 1 bar) in at least 90 % of the (row, head) pairs / elements
   (a scale of 1.0 read as 0.8 moves an element by a fifth of itself: the small ones stay inside any absolute bar);
3. the fence harness fails, with the message that names it, on a store one row block past a view, a skipped row block, a read of the row
   behind an input and a store into the V^T padding."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import attention_common as ac
from tests import rowchain_stages_common as rc
from tests.common import block_inputs, block_weights

CPU = torch.device("cpu")
POWER = 5.0


# ---------------------------------------------------------------------------------------------------- 1. the anchor
@pytest.mark.parametrize("name", ["tfm_320_cross", "tfm_320_self_only"])
def test_the_chained_stage_references_reproduce_the_block_fixture(golden_dir, name):
    z = np.load(os.path.join(golden_dir, "blocks.npz"))[name]
    x, _, ctx = block_inputs(name)
    B, C, H, W = x.shape
    ref = rc.BlockRef(block_weights(name), rounded=False)
    out = ref.block(x.permute(0, 2, 3, 1).reshape(-1, C).double(), B, ctx)
    got = out.view(B, H, W, C).permute(0, 3, 1, 2).numpy()
    err = float(np.abs(got - z).max() / np.abs(z).max())
    print(f"{name}: chained float64 stages vs the fp32 fixture: max-abs/scale {err:.3e}")
    assert got.shape == z.shape and err < 1e-5


# ---------------------------------------------------------------------------------------------------- 2. the named mistakes
@functools.lru_cache(maxsize=None)
def _ref(C, cross, zero=False):
    return rc.BlockRef(rc.block_sd(C, cross, zero))


def _bars(wrong, ref):
    """|wrong - ref| in units of the row bar (2e-3 |ref| + 2e-3 max(1, scale)), per element."""
    return (wrong - ref).abs() / (2e-3 * max(1.0, float(ref.abs().max())) + 2e-3 * ref.abs())


def _every_row(b, rows, what):
    per_row = b[rows].max(-1).values
    print(f"{what}: {float(per_row.min()):.1f} to {float(per_row.max()):.1f} bars over {len(per_row)} rows")
    assert len(per_row) and float(per_row.min()) > POWER, what


@functools.lru_cache(maxsize=None)
def _end(C, case):
    ref = _ref(C, True)
    _, _, HW, B, _ = rc.R2_CASES[case]
    return rc.end_reference(ref, B, HW, r2case=case)


@pytest.mark.parametrize("case", list(rc.R2_CASES))
@pytest.mark.parametrize("C", [320, 640])
def test_r2_xmin_off_by_one_shows_in_every_row_of_that_pixel_column(C, case):
    out_w, xmin, HW, B, bmod = rc.R2_CASES[case]
    pre = _end(C, case)
    good, r2, imgs = pre["r"]["out"], pre["r2"].double(), [b % bmod for b in range(B)]
    pix = torch.arange(B * HW) % HW % out_w
    for wrong_xmin, column in ((xmin + 1, xmin), (xmin - 1, xmin - 1)):
        if column < 0:
            continue                                    # (r2_xmin = 0: nothing lies left of it)
        wrong = rc.add_residual(pre["r"]["plain"], r2, B, out_w, wrong_xmin, imgs)
        rows = (pix == column).nonzero().flatten()
        assert len(rows) == B * HW // out_w
        _every_row(_bars(wrong, good), rows, f"C={C} {case}: r2_xmin {wrong_xmin} for {xmin}")


@pytest.mark.parametrize("case,mistake", [("w192", "bmod1"), ("w128", "bmod1"), ("w192", "neighbour"), ("w128", "neighbour"), ("w8", "neighbour")])
@pytest.mark.parametrize("C", [320, 640])
def test_a_wrong_residual_image_shows_in_every_row_that_takes_it(C, case, mistake):
    out_w, xmin, HW, B, bmod = rc.R2_CASES[case]
    pre = _end(C, case)
    right = [b % bmod for b in range(B)]
    imgs = [0] * B if mistake == "bmod1" else [(b + 1) % bmod for b in range(B)]
    wrong = rc.add_residual(pre["r"]["plain"], pre["r2"].double(), B, out_w, xmin, imgs)
    m = torch.arange(B * HW)
    concerned = torch.tensor([imgs[b] != right[b] for b in range(B)])[m // HW] & (m % HW % out_w >= xmin)
    _every_row(_bars(wrong, pre["r"]["out"]), concerned.nonzero().flatten(), f"C={C} {case}: residual image {imgs} for {right}")


@pytest.mark.parametrize("B,HW", [(3, 64), (2, 192)])
@pytest.mark.parametrize("C", [320, 640])
def test_groupnorm_statistics_of_the_neighbouring_image_show_in_every_row(C, B, HW):
    ref = _ref(C, True)
    x = rc.image_rows(11, B, HW, C).double()
    good, wrong = ref.stage_in(x, B), ref.stage_in(x, B, stats_of=[(b + 1) % B for b in range(B)])
    for label in ("h0", "q", "k", "v"):
        _every_row(_bars(wrong[label], good[label]), torch.arange(B * HW), f"C={C} B={B} HW={HW}: neighbour's GroupNorm statistics in {label}")


@pytest.mark.parametrize("B,HW", [(4, 64)])
@pytest.mark.parametrize("C", [320, 640])
def test_the_scale_of_the_neighbouring_image_shows_almost_everywhere(C, B, HW):
    ref = _ref(C, False, True)
    pre = rc.end_reference(ref, B, HW, zero_form="dev_b")
    alpha, _, _, _, scales = rc.alpha_table("dev_b", B, CPU)
    wrong = (pre["r"]["zero_unit"].view(B, HW, C) * alpha * scales.roll(1).double()[:, None, None]).reshape(-1, C)
    b = _bars(wrong, pre["r"]["zero"]).view(B, -1)
    share = (b > 1.0).double().mean(1)
    print(f"C={C}: neighbour's scale: worst {float(b.max()):.0f} bars, share of elements out of the bar per image {[round(float(s), 3) for s in share]}")
    assert float(b.max(1).values.min()) > POWER and float(share.min()) >= 0.9


@pytest.mark.parametrize("eps", [1e-6, 0.0])
@pytest.mark.parametrize("stage", ["mid", "end_unet", "end_blobnet"])
@pytest.mark.parametrize("C", [320, 640])
def test_a_wrong_layernorm_eps_shows_in_every_quiet_row(C, stage, eps):
    B, HW = 2, 64
    if stage == "mid":
        ref = _ref(C, True)
        a, res = rc.attn_and_res(21, B * HW, C, ref.v("transformer_blocks.0.attn1.to_out.0.bias"))
        good, wrong = (ref.stage_mid(a.double(), res.double(), e)["q"] for e in (rc.LN_EPS, eps))
    else:
        ref = _ref(C, stage == "end_unet", stage == "end_blobnet")
        a, res, x, _ = rc.end_inputs(ref, B, HW)
        good, wrong = (ref.stage_end(a.double(), res.double(), x.double(), B, ln_eps=e)["out"] for e in (rc.LN_EPS, eps))
    rows = rc.quiet_rows(B * HW)
    b = _bars(wrong, good)
    _every_row(b, rows, f"C={C} {stage}: ln_eps {eps:g} for {rc.LN_EPS:g}")
    loud = torch.ones(B * HW, dtype=torch.bool)
    loud[rows] = False
    assert float(b[loud].max()) < 0.1                   # (and nowhere else: at ordinary rows eps is invisible)


@pytest.mark.parametrize("T", [1, 17, 48, 77, 80])
@pytest.mark.parametrize("C", [320, 640])
def test_a_wrong_key_set_shows_in_nine_of_ten_row_head_pairs(C, T):
    """Key T - 1 dropped; key T added - the K row behind image b's keys is image b + 1's key 0 (the last image's: the fence), its V^T column
    is NaN padding: stated here with the next image's key 0 and V row 0, which a finite leak would look like."""
    B, HW, d = 3, 64, C // rc.HEADS
    ref = _ref(C, True)
    a, res, k, v = rc.midx_inputs(ref, B, HW, T)
    good = ref.stage_midx(a.double(), res.double(), k, v)
    q = good["q"].view(B, HW, C)
    wrongs = {"key T added": rc.attention(q, torch.cat([k, k.roll(-1, 0)[:, :1]], 1), torch.cat([v, v.roll(-1, 0)[:, :1]], 1))}
    if T > 1:
        wrongs["key T-1 dropped"] = rc.attention(q, k[:, :T - 1], v[:, :T - 1])
    gref = good["attn"].view(B, HW, C)
    for name, w in wrongs.items():
        b = ((w - gref).abs() / ac.bar(gref)).view(B * HW, rc.HEADS, d).max(-1).values
        share = float((b > 1.0).double().mean())
        print(f"C={C} T={T}: {name}: worst {float(b.max()):.0f} bars, {share:.3f} of the (row, head) pairs out of the bar")
        assert float(b.max()) > POWER and share >= 0.9


# ---------------------------------------------------------------------------------------------------- 3. the fence harness
B_, HW_, C_ = 2, 128, 320


def _in_prob(form="totals"):
    return rc.in_problem(_ref(C_, True), CPU, B_, HW_, form)


def _run(prob, mutation=None):
    prob.assert_inside()
    rc.emulate_in(_ref(C_, True), prob, mutation)
    return prob.verify()


@pytest.mark.parametrize("form", rc.IN_FORMS)
def test_the_correct_emulation_passes(form):
    prob = _in_prob(form)
    worst, checked = _run(prob)
    # (fp16 rounding of the outputs only; a row block of sentinels on either side of each output and the V^T padding columns)
    assert worst < 0.5 and checked == 2 * rc.GUARD * (C_ + 2 * C_ + HW_ + rc.VT_PAD) + B_ * C_ * rc.VT_PAD


M_ = B_ * HW_
CAUGHT = [("store_past", rf"\[h0\]: {64 * C_} elements outside the view were written, first at \(row {M_}, col 0\)"),
          ("skip_block", rf"\[q\|k\]: {64 * 2 * C_} elements of the view were left unwritten, first at \(row 64, col 0\)"),
          ("read_behind", rf"\[h0\]: {C_} non-finite elements in the view \(a leak\), first at \(row {M_ - 1}, col 0\)"),
          ("vt_pad", rf"\[V\^T\]: {B_ * C_ * 8} elements outside the view were written, first at \(row 0, col {HW_}\)")]


@pytest.mark.parametrize("mutation,message", CAUGHT, ids=[c[0] for c in CAUGHT])
def test_every_mistake_is_caught_by_name(mutation, message):
    with pytest.raises(AssertionError, match=message):
        _run(_in_prob(), mutation)


def test_every_mutation_of_the_emulation_is_exercised():
    assert sorted(c[0] for c in CAUGHT) == sorted(rc.MUTATIONS)


def test_the_input_fences_are_nan_and_the_totals_fence_is_poison():
    from blobctrl_amd.launch import decode_gn_tot
    prob = _in_prob()
    xv, tot = prob.views["x"], prob.views["gn_tot"]
    p = xv.parent.float()
    assert bool(torch.isnan(p[:xv.offset]).all()) and bool(torch.isnan(p[xv.offset + M_ * C_:]).all()) and bool(torch.isfinite(xv.valid().float()).all())
    d = decode_gn_tot(tot.parent)
    assert bool(torch.isnan(d[0]).all()) and bool(torch.isnan(d[-1]).all()) and bool(torch.isfinite(d[1:-1]).all())
    assert torch.allclose(d[1:-1], rc.gn_sums(xv.valid(), B_), rtol=1e-12, atol=1e-9)
    for form, n_read in (("dev", 1), ("dev_b", 4)):
        _, dev, idx, bstride, scales = rc.alpha_table(form, 4, CPU)
        assert int(torch.isfinite(dev.parent).sum()) == n_read
        read = dev.valid().flatten()[idx * max(bstride, 1) + (torch.arange(4) if bstride else torch.zeros(4, dtype=torch.long))]
        assert torch.equal(read, scales)
